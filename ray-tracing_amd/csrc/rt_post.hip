/*
 * rt_post.hip — the passes behind the render: the entry points of include/rt_adaptive.h, rt_denoise.h, rt_reproject.h, rt_motion.h
 * and rt_variance.h.  Their kernels are rt_adaptive.hip's, rt_denoise.hip's, rt_reproject.hip's and rt_variance.hip's, reached through
 * the *_launch.h headers; here are the argument checks, the scratch and the order on the joined main stream.  The two launches of
 * rt_kernels.h these passes need — the AOV pass and the frames of a tile list — are rt_context.hip's (aov_enqueue, adaptive_launch).
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include "rt_context.h"
#include "../../include/rt_aov.h"
#include "../../include/rt_denoise.h"
#include "../../include/rt_reproject.h"
#include "../../include/rt_variance.h"
#include "../../include/rt_adaptive.h"
#include "../../include/rt_motion.h"

#include "rt_denoise_launch.h"
#include "rt_denoise_math.h"
#include "rt_reproject_launch.h"
#include "rt_variance_launch.h"
#include "rt_adaptive_launch.h"

extern "C" {

/* ---- rt_adaptive_* (include/rt_adaptive.h): tile selection and the frames of a tile list ---------------------------------------
 * The kernels of the selection are rt_adaptive.hip's (rt_ad::enqueue_select); the frames themselves are adaptive_launch's. */
static int variance_images(RtContext* ctx);

static int adaptive_check_params(RtContext* ctx, const char* call, const RtAdaptiveParams* p, rt_ad_job* job)
{
    const char* why = "";
    const int rc = rt_ad::check_params(p, job, &why);
    return rc ? fail(ctx, rc, "%s: %s", call, why) : RT_OK;
}

int rt_adaptive_default_params(RtAdaptiveParams* out)
{
    if (!out) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_adaptive_default_params: out is null");
    memset(out, 0, sizeof(*out));
    out->struct_size = (uint32_t)sizeof(RtAdaptiveParams);
    out->threshold = 0.05f;
    out->darkFloor = 0.01f;
    out->minFrames = 8;
    out->maxFrames = 1024;
    return RT_OK;
}

int rt_adaptive_select_buffers(RtContext* ctx, const RtAdaptiveParams* p, int width, int height, const void* d_sum, const void* d_moments, void* d_tile_error,
                               void* d_tiles, void* d_counts)
{
    static const char* call = "rt_adaptive_select_buffers";
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    rt_ad_job job;
    int rc = adaptive_check_params(ctx, call, p, &job);
    if (rc) return rc;
    if ((rc = check_image_size(ctx, call, width, height, 1ll << 30))) return rc;
    const size_t n = (size_t)width * height, tiles = (size_t)rt_ad::tiles_total(width, height);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const struct { const char* what; const void* p; size_t bytes; bool out; } mem[5] = {
        {"d_sum", d_sum, n * 16, false}, {"d_moments", d_moments, n * 16, false}, {"d_tile_error", d_tile_error, tiles * 4, true},
        {"d_tiles", d_tiles, tiles * 4, true}, {"d_counts", d_counts, 16, true}};
    for (const auto& m : mem)
        if ((rc = check_device_range(ctx, call, m.what, m.p, m.bytes))) return rc;
    for (int i = 0; i < 5; i++)
        for (int j = i + 1; j < 5; j++)
            if ((mem[i].out || mem[j].out) && ranges_overlap(mem[i].p, mem[i].bytes, mem[j].p, mem[j].bytes))
                return fail(ctx, RT_ERR_INVALID_ARG, "%s: %s overlaps %s", call, mem[j].what, mem[i].what);
    RT_FLUSH(ctx);
    HIP_TRY(ctx, rt_ad::enqueue_select(joined(ctx), job, width, height, d_sum, d_moments, (float*)d_tile_error, (uint32_t*)d_tiles, (uint32_t*)d_counts));
    return RT_OK;
}

/* what every context call of this header starts with */
static int adaptive_check_context(RtContext* ctx, const char* call)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    if (ctx->W == 0) return fail(ctx, RT_ERR_STATE, "%s before rt_resize", call);
    return RT_OK;
}

/* The context's tile errors, list and counts exist, for its rows as they are now */
static int adaptive_buffers(RtContext* ctx)
{
    const long long total = rt_ad::tiles_total(ctx->W, ctx->localRows);
    if (!ctx->dAdCounts) HIP_TRY(ctx, hipMalloc(&ctx->dAdCounts, 16));
    if (ctx->adTilesTotal == total) return RT_OK;
    const size_t bytes = (size_t)(total > 0 ? total : 1) * 4;
    float* e = nullptr;
    uint32_t* t = nullptr;
    HIP_TRY(ctx, hipMalloc(&e, bytes));
    const hipError_t err = hipMalloc(&t, bytes);
    if (err != hipSuccess) {
        hipFree(e);
        HIP_TRY(ctx, err);
    }
    ctx->dAdTileError = e; /* (rt_resize freed the old pair) */
    ctx->dAdTiles = t;
    ctx->adTilesTotal = total;
    return RT_OK;
}

int rt_adaptive_select(RtContext* ctx, const RtAdaptiveParams* p, RtAdaptiveResult* out)
{
    static const char* call = "rt_adaptive_select";
    int rc = adaptive_check_context(ctx, call);
    if (rc) return rc;
    rt_ad_job job;
    if ((rc = adaptive_check_params(ctx, call, p, &job))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RT_FLUSH(ctx);
    if ((rc = variance_images(ctx))) return rc;
    if ((rc = adaptive_buffers(ctx))) return rc;
    ctx->adHaveList = ctx->adHaveErrors = false; /* until this selection has come back */
    hipStream_t st = joined(ctx);
    uint32_t counts[4] = {0, 0, 0, 0};
    if (ctx->adTilesTotal > 0)
        HIP_TRY(ctx, rt_ad::enqueue_select(st, job, ctx->W, ctx->localRows, accum_target(ctx), ctx->dMoments, ctx->dAdTileError, ctx->dAdTiles, ctx->dAdCounts));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    flush_timer(ctx);
    if ((rc = check_watchdog(ctx, ctx, call))) return rc;
    if (ctx->adTilesTotal > 0) HIP_TRY(ctx, hipMemcpy(counts, ctx->dAdCounts, sizeof(counts), hipMemcpyDeviceToHost));
    ctx->adTilesActive = counts[0];
    ctx->adPixelsActive = counts[1];
    ctx->adHaveList = ctx->adHaveErrors = true;
    if (out) {
        out->tiles_total = (uint32_t)ctx->adTilesTotal;
        out->tiles_active = counts[0];
        out->pixels_active = counts[1];
        out->reserved = 0;
    }
    return RT_OK;
}

int rt_adaptive_set_tiles(RtContext* ctx, const uint32_t* tiles, int n)
{
    static const char* call = "rt_adaptive_set_tiles";
    int rc = adaptive_check_context(ctx, call);
    if (rc) return rc;
    if (n < 0 || (n > 0 && !tiles)) return fail(ctx, RT_ERR_INVALID_ARG, "%s: %s", call, n < 0 ? "n < 0" : "tiles is null");
    uint32_t pixels = 0;
    if (const long long bad = rt_ad::check_tiles(tiles, n, ctx->W, ctx->localRows, &pixels))
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: entry %lld (tile %u) is not above its predecessor or not below tiles_total = %lld", call, bad - 1, tiles[bad - 1],
                    rt_ad::tiles_total(ctx->W, ctx->localRows));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RT_FLUSH(ctx);
    if ((rc = adaptive_buffers(ctx))) return rc;
    ctx->adHaveList = false;
    if ((rc = stage_upload(ctx, ctx->dAdTiles, tiles, (size_t)n * 4))) return rc; /* stream-ordered: behind the launches that read the old list */
    ctx->adTilesActive = (uint32_t)n;
    ctx->adPixelsActive = pixels;
    ctx->adHaveList = true;
    return RT_OK;
}

int rt_adaptive_read_tiles(RtContext* ctx, uint32_t* tiles, int capacity, int* n)
{
    static const char* call = "rt_adaptive_read_tiles";
    int rc = adaptive_check_context(ctx, call);
    if (rc) return rc;
    if (!n) return fail(ctx, RT_ERR_INVALID_ARG, "%s: n is null", call);
    if (!ctx->adHaveList) return fail(ctx, RT_ERR_STATE, "%s: no tile list (rt_adaptive_select or rt_adaptive_set_tiles makes one; rt_resize drops it)", call);
    *n = (int)ctx->adTilesActive;
    if (!tiles) return RT_OK;
    if (capacity < (int)ctx->adTilesActive) return fail(ctx, RT_ERR_INVALID_ARG, "%s: the list has %u entries, capacity is %d", call, ctx->adTilesActive, capacity);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RT_FLUSH(ctx);
    HIP_TRY(ctx, hipStreamSynchronize(joined(ctx)));
    flush_timer(ctx);
    if (ctx->adTilesActive) HIP_TRY(ctx, hipMemcpy(tiles, ctx->dAdTiles, (size_t)ctx->adTilesActive * 4, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_adaptive_read_tile_error(RtContext* ctx, float* err, size_t bytes)
{
    static const char* call = "rt_adaptive_read_tile_error";
    int rc = adaptive_check_context(ctx, call);
    if (rc) return rc;
    if (!ctx->adHaveErrors) return fail(ctx, RT_ERR_STATE, "%s: no rt_adaptive_select since the last rt_resize", call);
    if (bytes != (size_t)ctx->adTilesTotal * 4 || (!err && bytes))
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: need exactly %zu bytes (%lld tiles x 4), got %zu%s", call, (size_t)ctx->adTilesTotal * 4, ctx->adTilesTotal, bytes,
                    err ? "" : " and a null pointer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RT_FLUSH(ctx);
    HIP_TRY(ctx, hipStreamSynchronize(joined(ctx)));
    flush_timer(ctx);
    if (bytes) HIP_TRY(ctx, hipMemcpy(err, ctx->dAdTileError, bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_adaptive_render_frames(RtContext* ctx, int n)
{
    static const char* call = "rt_adaptive_render_frames";
    int rc = check_renderable(ctx);
    if (rc) return rc;
    if (n < 0) return fail(ctx, RT_ERR_INVALID_ARG, "%s: n < 0", call);
    if (!ctx->params.accumulate) return fail(ctx, RT_ERR_STATE, "%s: params.accumulate is 0: a frame that adds nothing has nothing to be selective about", call);
    if (!ctx->adHaveList) return fail(ctx, RT_ERR_STATE, "%s: no tile list (rt_adaptive_select or rt_adaptive_set_tiles makes one; rt_resize drops it)", call);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RT_FLUSH(ctx);
    if (ctx->adTilesActive == 0) { /* nothing to render: the frames still count */
        ctx->frame += n;
        return RT_OK;
    }
    bool fuse = ctx->fuseFrames;
    while (n > 0) {
        const int k = fuse ? (n < ctx->fuseCap ? n : ctx->fuseCap) : 1;
        bool unstaged = false;
        if ((rc = adaptive_launch(ctx, ctx->frame, k, &unstaged))) return rc;
        if (unstaged) { /* no slab: one launch per frame, the same bits */
            fuse = false;
            continue;
        }
        ctx->frame += k;
        n -= k;
    }
    return RT_OK;
}

/* ---- rt_denoise_buffers / rt_denoise / rt_denoise_to_device (include/rt_denoise.h) --------------------------------------------
 * The kernels are rt_denoise.hip's (rt_dn::enqueue); here are the argument checks, the scratch and the order on the joined main
 * stream.  The two context calls run the AOV pass of rt_render_aov_to_device into library-owned records first, with that pass's own
 * watchdog word and its reporting. */
static int denoise_check_params(RtContext* ctx, const char* call, const RtDenoiseParams* p, rt_dn::Job* job)
{
    if (!p) return fail(ctx, RT_ERR_INVALID_ARG, "%s: null parameters", call);
    if (p->struct_size != sizeof(RtDenoiseParams))
        return fail(ctx, RT_ERR_ABI_MISMATCH, "%s: RtDenoiseParams.struct_size is %u, this library's is %zu", call, p->struct_size, sizeof(RtDenoiseParams));
    if (p->iterations < 0 || p->iterations > RT_DENOISE_MAX_ITERATIONS)
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: iterations %d outside 0..%d", call, p->iterations, RT_DENOISE_MAX_ITERATIONS);
    const float sig[3] = {p->sigmaColour, p->sigmaNormal, p->sigmaPlane};
    for (float s : sig)
        if (!(s > 0.0f) || !rt_dn_finite(s)) return fail(ctx, RT_ERR_INVALID_ARG, "%s: every sigma must be finite and > 0", call);
    if (!rt_dn_finite(p->scale)) return fail(ctx, RT_ERR_INVALID_ARG, "%s: scale is not finite", call);
    if (p->reserved != 0) return fail(ctx, RT_ERR_INVALID_ARG, "%s: reserved must be 0", call);
    job->iterations = p->iterations;
    job->demodulate = p->demodulate != 0;
    job->scale = p->scale;
    job->aC = rt_dn_inv_sq(p->sigmaColour);
    job->aN = rt_dn_inv_sq(p->sigmaNormal);
    job->aP = rt_dn_inv_sq(p->sigmaPlane);
    /* a sigma so small that 1 / sigma^2 (for the colour: times 4^i in the last pass) is infinite would turn the centre tap's e = 0 * inf into NaN */
    if (!rt_dn_finite(job->aN) || !rt_dn_finite(job->aP) || !rt_dn_finite(rt_dn_colour_scale(job->aC, p->iterations > 0 ? p->iterations - 1 : 0)))
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: a sigma is too small: 1 / sigma^2 is not finite in fp32", call);
    return RT_OK;
}

int rt_denoise_default_params(RtDenoiseParams* out)
{
    if (!out) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_denoise_default_params: out is null");
    memset(out, 0, sizeof(*out));
    out->struct_size = (uint32_t)sizeof(RtDenoiseParams);
    out->iterations = 5;
    out->sigmaColour = 4.0f;
    out->sigmaNormal = 0.25f;
    out->sigmaPlane = 0.1f;
    out->demodulate = 1;
    out->scale = 1.0f;
    return RT_OK;
}

int rt_denoise_buffers(RtContext* ctx, const RtDenoiseParams* p, int width, int height, const void* d_rgba_in, const void* d_aov, void* d_rgba_out)
{
    static const char* call = "rt_denoise_buffers";
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    rt_dn::Job job;
    int rc = denoise_check_params(ctx, call, p, &job);
    if (rc) return rc;
    if ((rc = check_image_size(ctx, call, width, height, (long long)INT32_MAX / 2))) return rc;
    if ((rc = check_whole_image(ctx, call, "the filter", "gather, then rt_denoise_buffers"))) return rc;
    const size_t n = (size_t)width * height;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = check_device_range(ctx, call, "d_rgba_in", d_rgba_in, n * 16))) return rc;
    if ((rc = check_device_range(ctx, call, "d_aov", d_aov, n * sizeof(RtPixelAov)))) return rc;
    if ((rc = check_device_range(ctx, call, "d_rgba_out", d_rgba_out, n * 16))) return rc;
    if (ranges_overlap(d_rgba_out, n * 16, d_rgba_in, n * 16) || ranges_overlap(d_rgba_out, n * 16, d_aov, n * sizeof(RtPixelAov)))
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: d_rgba_out overlaps an input", call);
    RT_FLUSH(ctx);
    if ((rc = grow_scratch(ctx, &ctx->dDnScratch, &ctx->dnScratchBytes, rt_dn::scratch_bytes(n)))) return rc;
    job.W = width;
    job.H = height;
    HIP_TRY(ctx, rt_dn::enqueue(joined(ctx), job, d_rgba_in, d_aov, d_rgba_out, ctx->dDnScratch));
    return RT_OK;
}

/* how rt_denoise and rt_denoise_variance end, their filter enqueued into ctx->dDisplay behind its AOV pass: the pass's word, then the
 * context's, then the image */
static int filtered_to_host(RtContext* ctx, const char* call, float* rgba, size_t bytes)
{
    HIP_TRY(ctx, hipStreamSynchronize(joined(ctx)));
    flush_timer(ctx);
    unsigned long long fired = 0;
    if (int rc = side_fired(ctx, ctx->side[SIDE_AOV], &fired)) return rc;
    if (fired) return watchdog_failure(ctx, call, fired);
    if (int rc = check_watchdog(ctx, ctx, call)) return rc;
    HIP_TRY(ctx, hipMemcpy(rgba, ctx->dDisplay, bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

/* what rt_denoise and rt_denoise_to_device share: checks, the AOV pass, the filter from the context's image into dOut (device) */
static int denoise_check_context_call(RtContext* ctx, const char* call, const RtDenoiseParams* p, int aov_frame, const void* out, size_t bytes, rt_dn::Job* job)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    int rc = denoise_check_params(ctx, call, p, job);
    if (rc) return rc;
    if (aov_frame < 1) return fail(ctx, RT_ERR_INVALID_ARG, "%s: aov_frame %d < 1 (the first frame after a reset is 1)", call, aov_frame);
    if ((rc = check_renderable(ctx))) return rc;
    if ((rc = check_whole_image(ctx, call, "the filter", "gather, then rt_denoise_buffers"))) return rc;
    if ((rc = check_rows_buffer(ctx, call, 16, out, bytes))) return rc;
    job->W = ctx->W;
    job->H = ctx->localRows;
    return RT_OK;
}

static int denoise_enqueue_context_call(RtContext* ctx, const rt_dn::Job& job, int use_accumulated, int aov_frame, void* dOut)
{
    const size_t n = (size_t)job.W * job.H;
    int rc;
    if ((rc = grow_scratch(ctx, &ctx->dDnScratch, &ctx->dnScratchBytes, rt_dn::scratch_bytes(n)))) return rc;
    if ((rc = grow_scratch(ctx, &ctx->dDnAov, &ctx->dnAovBytes, n * sizeof(RtPixelAov)))) return rc;
    if ((rc = aov_enqueue(ctx, aov_frame, ctx->dDnAov))) return rc;
    HIP_TRY(ctx, rt_dn::enqueue(joined(ctx), job, image_target(ctx, use_accumulated), ctx->dDnAov, dOut, ctx->dDnScratch));
    return RT_OK;
}

int rt_denoise(RtContext* ctx, const RtDenoiseParams* p, int use_accumulated, int aov_frame, float* rgba, size_t bytes)
{
    static const char* call = "rt_denoise";
    rt_dn::Job job;
    int rc = denoise_check_context_call(ctx, call, p, aov_frame, rgba, bytes, &job);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RT_FLUSH(ctx);
    if ((rc = side_settle(ctx, ctx->side[SIDE_AOV], call))) return rc;
    if (!bytes) return RT_OK;
    if ((rc = grow_scratch(ctx, &ctx->dDisplay, &ctx->displayBytes, bytes))) return rc;
    if ((rc = denoise_enqueue_context_call(ctx, job, use_accumulated, aov_frame, ctx->dDisplay))) return rc;
    return filtered_to_host(ctx, call, rgba, bytes);
}

int rt_denoise_to_device(RtContext* ctx, const RtDenoiseParams* p, int use_accumulated, int aov_frame, void* d_rgba, size_t bytes)
{
    static const char* call = "rt_denoise_to_device";
    rt_dn::Job job;
    int rc = denoise_check_context_call(ctx, call, p, aov_frame, d_rgba, bytes, &job);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = check_image_out(ctx, call, d_rgba, bytes, image_target(ctx, use_accumulated), "the source image"))) return rc;
    RT_FLUSH(ctx);
    if ((rc = side_settle(ctx, ctx->side[SIDE_AOV], call))) return rc;
    if (!bytes) return RT_OK;
    if ((rc = denoise_enqueue_context_call(ctx, job, use_accumulated, aov_frame, d_rgba))) return rc;
    ctx->side[SIDE_AOV].unreported = true;
    return RT_OK;
}

/* ---- rt_reproject_buffers / rt_reproject_accumulated / rt_resolve* (include/rt_reproject.h) and their *_moving forms (include/rt_motion.h)
 * The kernels are rt_reproject.hip's (rt_rp::enqueue*); here are the argument checks, the scratch and the order.  Everything runs on the
 * joined main stream (rt_launch_order.h, join): behind every frame either render stream holds, and — join() re-arms the fork — in front
 * of every frame requested later, which is how rt_reset_accumulation and rt_write_accumulated order their write of the accumulator.
 * The scratch is the denoiser's: its colour images hold the reprojected image, its records the current view's; both are only ever used
 * by work on this one stream. */
static int reproject_check_params(RtContext* ctx, const char* call, const RtReprojectParams* p, rt_rp_job* job)
{
    if (!p) return fail(ctx, RT_ERR_INVALID_ARG, "%s: null parameters", call);
    if (p->struct_size != sizeof(RtReprojectParams))
        return fail(ctx, RT_ERR_ABI_MISMATCH, "%s: RtReprojectParams.struct_size is %u, this library's is %zu", call, p->struct_size, sizeof(RtReprojectParams));
    if (!(p->maxPlaneDistance >= 0.0f) || !rt_rp_finite(p->maxPlaneDistance)) return fail(ctx, RT_ERR_INVALID_ARG, "%s: maxPlaneDistance must be finite and >= 0", call);
    if (!rt_rp_finite(p->minNormalDot)) return fail(ctx, RT_ERR_INVALID_ARG, "%s: minNormalDot is not finite", call);
    if (!(p->maxHistory > 0.0f) || !rt_rp_finite(p->maxHistory)) return fail(ctx, RT_ERR_INVALID_ARG, "%s: maxHistory must be finite and > 0", call);
    if (p->flags & ~RT_REPROJECT_FLAG_GLASS) return fail(ctx, RT_ERR_INVALID_ARG, "%s: flags 0x%x: only bit 0 is defined", call, p->flags);
    if (p->reserved != 0) return fail(ctx, RT_ERR_INVALID_ARG, "%s: reserved must be 0", call);
    for (int r = 0; r < 3; r++) {
        job->R[r] = p->prevCamLocalToWorld[r];
        job->U[r] = p->prevCamLocalToWorld[4 + r];
        job->F[r] = p->prevCamLocalToWorld[8 + r];
        job->O[r] = p->prevCamLocalToWorld[12 + r];
    }
    job->pw = p->prevViewParams[0];
    job->ph = p->prevViewParams[1];
    job->fd = p->prevViewParams[2];
    job->maxPlaneDistance = p->maxPlaneDistance;
    job->minNormalDot = p->minNormalDot;
    job->maxHistory = p->maxHistory;
    job->glass = (int)(p->flags & RT_REPROJECT_FLAG_GLASS);
    return RT_OK;
}

int rt_reproject_default_params(RtReprojectParams* out)
{
    if (!out) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_reproject_default_params: out is null");
    memset(out, 0, sizeof(*out));
    out->struct_size = (uint32_t)sizeof(RtReprojectParams);
    out->maxPlaneDistance = 0.1f;
    out->minNormalDot = 0.9f;
    out->maxHistory = 256.0f;
    return RT_OK;
}

/* The table of a *_moving call (nullptr: a static call, nothing to check): its size, its memory, and no overlap with what the call
 * writes — `out` (outBytes) and, when given, `out2` (out2Bytes). */
struct MotionArg {
    bool moving;
    const void* d;
    int n;
};

static int check_motion_table(RtContext* ctx, const char* call, const MotionArg& mo, const void* out, size_t outBytes, const void* out2 = nullptr, size_t out2Bytes = 0)
{
    if (!mo.moving) return RT_OK;
    if (mo.n < 0 || mo.n > (1 << 24)) return fail(ctx, RT_ERR_INVALID_ARG, "%s: n_objects %d outside 0..2^24", call, mo.n);
    if (mo.n == 0) return RT_OK; /* d_motion is not looked at */
    const size_t bytes = (size_t)mo.n * sizeof(RtObjectMotion);
    if (int rc = check_device_range(ctx, call, "d_motion", mo.d, bytes)) return rc;
    if (ranges_overlap(mo.d, bytes, out, outBytes) || (out2 && ranges_overlap(mo.d, bytes, out2, out2Bytes)))
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: d_motion overlaps an output", call);
    return RT_OK;
}

/* the static kernel for the static calls (their bits and their time stay theirs), the table's kernel for the *_moving calls */
static hipError_t reproject_enqueue(hipStream_t st, const rt_rp_job& job, const void* dPrevRgba, const void* dPrevAov, const void* dCurAov, const MotionArg& mo, void* dOut)
{
    if (!mo.moving) return rt_rp::enqueue(st, job, dPrevRgba, dPrevAov, dCurAov, dOut);
    return rt_rp::enqueue_moving(st, job, dPrevRgba, dPrevAov, dCurAov, mo.n ? mo.d : nullptr, mo.n, dOut);
}

static int reproject_buffers_call(RtContext* ctx, const char* call, const RtReprojectParams* p, int width, int height, const void* d_prev_rgba, const void* d_prev_aov,
                                  const void* d_cur_aov, const MotionArg& mo, void* d_out_rgba)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    rt_rp_job job;
    int rc = reproject_check_params(ctx, call, p, &job);
    if (rc) return rc;
    if ((rc = check_image_size(ctx, call, width, height, 1ll << 30))) return rc;
    if ((rc = check_whole_image(ctx, call, "reprojection", "gather first"))) return rc;
    const size_t n = (size_t)width * height;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = check_device_range(ctx, call, "d_prev_rgba", d_prev_rgba, n * 16))) return rc;
    if ((rc = check_device_range(ctx, call, "d_prev_aov", d_prev_aov, n * sizeof(RtPixelAov)))) return rc;
    if ((rc = check_device_range(ctx, call, "d_cur_aov", d_cur_aov, n * sizeof(RtPixelAov)))) return rc;
    if ((rc = check_device_range(ctx, call, "d_out_rgba", d_out_rgba, n * 16))) return rc;
    if (ranges_overlap(d_out_rgba, n * 16, d_prev_rgba, n * 16) || ranges_overlap(d_out_rgba, n * 16, d_prev_aov, n * sizeof(RtPixelAov)) ||
        ranges_overlap(d_out_rgba, n * 16, d_cur_aov, n * sizeof(RtPixelAov)))
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: d_out_rgba overlaps an input", call);
    if ((rc = check_motion_table(ctx, call, mo, d_out_rgba, n * 16))) return rc;
    RT_FLUSH(ctx);
    job.W = width;
    job.H = height;
    HIP_TRY(ctx, reproject_enqueue(joined(ctx), job, d_prev_rgba, d_prev_aov, d_cur_aov, mo, d_out_rgba));
    return RT_OK;
}

int rt_reproject_buffers(RtContext* ctx, const RtReprojectParams* p, int width, int height, const void* d_prev_rgba, const void* d_prev_aov, const void* d_cur_aov,
                         void* d_out_rgba)
{
    return reproject_buffers_call(ctx, "rt_reproject_buffers", p, width, height, d_prev_rgba, d_prev_aov, d_cur_aov, MotionArg{false, nullptr, 0}, d_out_rgba);
}

int rt_reproject_buffers_moving(RtContext* ctx, const RtReprojectParams* p, int width, int height, const void* d_prev_rgba, const void* d_prev_aov, const void* d_cur_aov,
                                const void* d_motion, int n_objects, void* d_out_rgba)
{
    return reproject_buffers_call(ctx, "rt_reproject_buffers_moving", p, width, height, d_prev_rgba, d_prev_aov, d_cur_aov, MotionArg{true, d_motion, n_objects}, d_out_rgba);
}

/* aov_frame: >= 1, or RT_AOV_CENTRE where the call admits it (centreAllowed) */
static int reproject_accumulated_call(RtContext* ctx, const char* call, const RtReprojectParams* p, const void* d_prev_aov, int aov_frame, bool centreAllowed,
                                      const MotionArg& mo, void* d_cur_aov_out)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    rt_rp_job job;
    int rc = reproject_check_params(ctx, call, p, &job);
    if (rc) return rc;
    if (centreAllowed ? aov_frame < 0 : aov_frame < 1)
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: aov_frame %d < %d (the first frame after a reset is 1%s)", call, aov_frame, centreAllowed ? 0 : 1,
                    centreAllowed ? "; RT_AOV_CENTRE, 0, is the pixel-centre pass" : "");
    if ((rc = check_renderable(ctx))) return rc;
    if ((rc = check_whole_image(ctx, call, "reprojection", "gather, then rt_reproject_buffers"))) return rc;
    job.W = ctx->W;
    job.H = ctx->localRows;
    const size_t n = (size_t)job.W * job.H, recBytes = n * sizeof(RtPixelAov);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    float* const accum = accum_target(ctx);
    if (!d_prev_aov) return fail(ctx, RT_ERR_INVALID_ARG, "%s: d_prev_aov is null", call);
    if ((uintptr_t)d_prev_aov & 15) return fail(ctx, RT_ERR_INVALID_ARG, "%s: d_prev_aov must be 16-byte aligned", call);
    if ((uintptr_t)d_cur_aov_out & 15) return fail(ctx, RT_ERR_INVALID_ARG, "%s: d_cur_aov_out must be 16-byte aligned", call);
    if (n) {
        if ((rc = check_device_range(ctx, call, "d_prev_aov", d_prev_aov, recBytes))) return rc;
        if (ranges_overlap(d_prev_aov, recBytes, accum, n * 16)) return fail(ctx, RT_ERR_INVALID_ARG, "%s: d_prev_aov overlaps AccumulatedRender", call);
        if (d_cur_aov_out) {
            if ((rc = check_device_range(ctx, call, "d_cur_aov_out", d_cur_aov_out, recBytes))) return rc;
            if (ranges_overlap(d_cur_aov_out, recBytes, d_prev_aov, recBytes) || ranges_overlap(d_cur_aov_out, recBytes, accum, n * 16))
                return fail(ctx, RT_ERR_INVALID_ARG, "%s: d_cur_aov_out overlaps d_prev_aov or AccumulatedRender", call);
        }
    }
    if ((rc = check_motion_table(ctx, call, mo, accum, n * 16, d_cur_aov_out, recBytes))) return rc;
    RT_FLUSH(ctx);
    if ((rc = side_settle(ctx, ctx->side[SIDE_AOV], call))) return rc;
    if (!n) return RT_OK;
    if ((rc = grow_scratch(ctx, &ctx->dDnScratch, &ctx->dnScratchBytes, n * 16))) return rc;
    if ((rc = grow_scratch(ctx, &ctx->dDnAov, &ctx->dnAovBytes, recBytes))) return rc;
    if ((rc = aov_enqueue(ctx, aov_frame, ctx->dDnAov))) return rc;
    ctx->side[SIDE_AOV].unreported = true;
    hipStream_t st = joined(ctx);
    if (d_cur_aov_out) HIP_TRY(ctx, hipMemcpyAsync(d_cur_aov_out, ctx->dDnAov, recBytes, hipMemcpyDeviceToDevice, st));
    HIP_TRY(ctx, reproject_enqueue(st, job, accum, d_prev_aov, ctx->dDnAov, mo, ctx->dDnScratch));
    /* over the accumulator, unless the pass's watchdog fired: the device reads the pass's own word, the host reports it later */
    HIP_TRY(ctx, rt_rp::enqueue_commit(st, ctx->dDnScratch, accum, n, ctx->side[SIDE_AOV].words + kWatchdogWord));
    return RT_OK;
}

int rt_reproject_accumulated(RtContext* ctx, const RtReprojectParams* p, const void* d_prev_aov, int aov_frame, void* d_cur_aov_out)
{
    return reproject_accumulated_call(ctx, "rt_reproject_accumulated", p, d_prev_aov, aov_frame, false, MotionArg{false, nullptr, 0}, d_cur_aov_out);
}

int rt_reproject_accumulated_moving(RtContext* ctx, const RtReprojectParams* p, const void* d_prev_aov, int aov_frame, const void* d_motion, int n_objects,
                                    void* d_cur_aov_out)
{
    return reproject_accumulated_call(ctx, "rt_reproject_accumulated_moving", p, d_prev_aov, aov_frame, true, MotionArg{true, d_motion, n_objects}, d_cur_aov_out);
}

/* Pure host code: no context, no device (include/rt_motion.h states the arithmetic; rt_motion_math.h is it) */
int rt_motion_from_scene(const RtSphere* prev_spheres, const RtSphere* cur_spheres, int n_spheres, const RtModel* prev_models, const RtModel* cur_models, int n_models,
                         RtObjectMotion* out)
{
    static const char* call = "rt_motion_from_scene";
    if (n_spheres < 0 || n_models < 0) return fail(nullptr, RT_ERR_INVALID_ARG, "%s: a negative count", call);
    if (n_spheres && (!prev_spheres || !cur_spheres)) return fail(nullptr, RT_ERR_INVALID_ARG, "%s: null spheres with n_spheres %d", call, n_spheres);
    if (n_models && (!prev_models || !cur_models)) return fail(nullptr, RT_ERR_INVALID_ARG, "%s: null models with n_models %d", call, n_models);
    if ((n_spheres || n_models) && !out) return fail(nullptr, RT_ERR_INVALID_ARG, "%s: out is null", call);
    for (int i = 0; i < n_spheres; i++) rt_mo_sphere_entry(prev_spheres[i].centre, cur_spheres[i].centre, out[i].m);
    for (int j = 0; j < n_models; j++) rt_mo_model_entry(prev_models[j].localToWorld, cur_models[j].worldToLocal, out[(size_t)n_spheres + j].m);
    return RT_OK;
}

int rt_resolve_buffers(RtContext* ctx, int width, int height, const void* d_rgba_sum, void* d_rgba_out)
{
    static const char* call = "rt_resolve_buffers";
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    int rc = check_image_size(ctx, call, width, height, 1ll << 30);
    if (rc) return rc;
    const size_t n = (size_t)width * height;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = check_device_range(ctx, call, "d_rgba_sum", d_rgba_sum, n * 16))) return rc;
    if ((rc = check_device_range(ctx, call, "d_rgba_out", d_rgba_out, n * 16))) return rc;
    if (d_rgba_out != d_rgba_sum && ranges_overlap(d_rgba_out, n * 16, d_rgba_sum, n * 16))
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: d_rgba_out overlaps d_rgba_sum without being it (in place means the same pointer)", call);
    RT_FLUSH(ctx);
    HIP_TRY(ctx, rt_rp::enqueue_resolve(joined(ctx), d_rgba_sum, d_rgba_out, n));
    return RT_OK;
}

static int resolve_check_call(RtContext* ctx, const char* call, const void* out, size_t bytes)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    if (ctx->W == 0) return fail(ctx, RT_ERR_STATE, "%s before rt_resize", call);
    return check_rows_buffer(ctx, call, 16, out, bytes);
}

int rt_resolve(RtContext* ctx, float* rgba, size_t bytes)
{
    static const char* call = "rt_resolve";
    int rc = resolve_check_call(ctx, call, rgba, bytes);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RT_FLUSH(ctx);
    if (bytes) {
        if ((rc = grow_scratch(ctx, &ctx->dDisplay, &ctx->displayBytes, bytes))) return rc;
        HIP_TRY(ctx, rt_rp::enqueue_resolve(joined(ctx), accum_target(ctx), ctx->dDisplay, bytes / 16));
    }
    HIP_TRY(ctx, hipStreamSynchronize(joined(ctx)));
    flush_timer(ctx);
    /* a device AOV pass completes here: a watchdog that fired in rt_reproject_accumulated's pass left the accumulator as it was, and the
     * caller of this host read must not take its resolve for the reprojected image */
    if ((rc = side_report(ctx, ctx->side[SIDE_AOV], call))) return rc;
    if ((rc = check_watchdog(ctx, ctx, call))) return rc;
    if (bytes) HIP_TRY(ctx, hipMemcpy(rgba, ctx->dDisplay, bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_resolve_to_device(RtContext* ctx, void* d_rgba, size_t bytes)
{
    static const char* call = "rt_resolve_to_device";
    int rc = resolve_check_call(ctx, call, d_rgba, bytes);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = check_image_out(ctx, call, d_rgba, bytes, accum_target(ctx), "AccumulatedRender"))) return rc;
    RT_FLUSH(ctx);
    if (!bytes) return RT_OK;
    HIP_TRY(ctx, rt_rp::enqueue_resolve(joined(ctx), accum_target(ctx), d_rgba, bytes / 16));
    return RT_OK;
}

/* ---- rt_moments_update_buffers / rt_denoise_variance* / rt_variance_* (include/rt_variance.h) ------------------------------------
 * The kernels are rt_variance.hip's (rt_vr::enqueue*) and, for the carry, rt_reproject.hip's; here are the argument checks, the
 * context's moments and the order on the joined main stream.  The filter's scratch is the plain filter's (same layout), with the
 * resolved image of the two context calls behind it. */
static int variance_check_params(RtContext* ctx, const char* call, const RtVarianceDenoiseParams* p, rt_vr::Job* job)
{
    if (!p) return fail(ctx, RT_ERR_INVALID_ARG, "%s: null parameters", call);
    if (p->struct_size != sizeof(RtVarianceDenoiseParams))
        return fail(ctx, RT_ERR_ABI_MISMATCH, "%s: RtVarianceDenoiseParams.struct_size is %u, this library's is %zu", call, p->struct_size, sizeof(RtVarianceDenoiseParams));
    if (p->iterations < 0 || p->iterations > RT_DENOISE_MAX_ITERATIONS)
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: iterations %d outside 0..%d", call, p->iterations, RT_DENOISE_MAX_ITERATIONS);
    const float sig[3] = {p->sigmaLuminance, p->sigmaNormal, p->sigmaPlane};
    for (float s : sig)
        if (!(s > 0.0f) || !rt_dn_finite(s)) return fail(ctx, RT_ERR_INVALID_ARG, "%s: every sigma must be finite and > 0", call);
    if (!rt_dn_finite(p->scale)) return fail(ctx, RT_ERR_INVALID_ARG, "%s: scale is not finite", call);
    if (!(p->unknownVariance >= 0.0f) || !rt_dn_finite(p->unknownVariance)) return fail(ctx, RT_ERR_INVALID_ARG, "%s: unknownVariance must be finite and >= 0", call);
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(ctx, RT_ERR_INVALID_ARG, "%s: reserved must be 0", call);
    job->iterations = p->iterations;
    job->demodulate = p->demodulate != 0;
    job->scale = p->scale;
    job->unknownVariance = p->unknownVariance;
    job->sigmaLuminance = p->sigmaLuminance;
    job->aN = rt_dn_inv_sq(p->sigmaNormal);
    job->aP = rt_dn_inv_sq(p->sigmaPlane);
    if (!rt_dn_finite(job->aN) || !rt_dn_finite(job->aP)) /* the centre tap's e = 0 * inf would be NaN, as in denoise_check_params */
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: a sigma is too small: 1 / sigma^2 is not finite in fp32", call);
    return RT_OK;
}

int rt_denoise_variance_default_params(RtVarianceDenoiseParams* out)
{
    if (!out) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_denoise_variance_default_params: out is null");
    memset(out, 0, sizeof(*out));
    out->struct_size = (uint32_t)sizeof(RtVarianceDenoiseParams);
    out->iterations = 5;
    out->sigmaLuminance = 4.0f;
    out->sigmaNormal = 0.25f;
    out->sigmaPlane = 0.1f;
    out->demodulate = 1;
    out->scale = 1.0f;
    out->unknownVariance = 1.0f;
    return RT_OK;
}

int rt_moments_update_buffers(RtContext* ctx, int width, int height, const void* d_sum, void* d_snapshot, void* d_moments, int rebase)
{
    static const char* call = "rt_moments_update_buffers";
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    int rc = check_image_size(ctx, call, width, height, 1ll << 30);
    if (rc) return rc;
    const size_t n = (size_t)width * height;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = check_device_range(ctx, call, "d_sum", d_sum, n * 16))) return rc;
    if ((rc = check_device_range(ctx, call, "d_snapshot", d_snapshot, n * 16))) return rc;
    if ((rc = check_device_range(ctx, call, "d_moments", d_moments, n * 16))) return rc;
    if (ranges_overlap(d_sum, n * 16, d_snapshot, n * 16) || ranges_overlap(d_sum, n * 16, d_moments, n * 16) || ranges_overlap(d_snapshot, n * 16, d_moments, n * 16))
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: two of the three images overlap", call);
    RT_FLUSH(ctx);
    HIP_TRY(ctx, rt_vr::enqueue_update(joined(ctx), d_sum, d_snapshot, d_moments, n, rebase));
    return RT_OK;
}

int rt_denoise_variance_buffers(RtContext* ctx, const RtVarianceDenoiseParams* p, int width, int height, const void* d_rgba_in, const void* d_moments, const void* d_aov,
                                void* d_rgba_out)
{
    static const char* call = "rt_denoise_variance_buffers";
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    rt_vr::Job job;
    int rc = variance_check_params(ctx, call, p, &job);
    if (rc) return rc;
    if ((rc = check_image_size(ctx, call, width, height, 1ll << 30))) return rc;
    if ((rc = check_whole_image(ctx, call, "the filter", "gather, then rt_denoise_variance_buffers"))) return rc;
    const size_t n = (size_t)width * height;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = check_device_range(ctx, call, "d_rgba_in", d_rgba_in, n * 16))) return rc;
    if ((rc = check_device_range(ctx, call, "d_moments", d_moments, n * 16))) return rc;
    if ((rc = check_device_range(ctx, call, "d_aov", d_aov, n * sizeof(RtPixelAov)))) return rc;
    if ((rc = check_device_range(ctx, call, "d_rgba_out", d_rgba_out, n * 16))) return rc;
    if (ranges_overlap(d_rgba_out, n * 16, d_rgba_in, n * 16) || ranges_overlap(d_rgba_out, n * 16, d_moments, n * 16) ||
        ranges_overlap(d_rgba_out, n * 16, d_aov, n * sizeof(RtPixelAov)))
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: d_rgba_out overlaps an input", call);
    RT_FLUSH(ctx);
    if ((rc = grow_scratch(ctx, &ctx->dDnScratch, &ctx->dnScratchBytes, rt_vr::scratch_bytes(n)))) return rc;
    job.W = width;
    job.H = height;
    HIP_TRY(ctx, rt_vr::enqueue(joined(ctx), job, d_rgba_in, d_moments, d_aov, d_rgba_out, ctx->dDnScratch));
    return RT_OK;
}

/* The context's moments and snapshot exist, for its rows as they are now; fresh ones are all zero (stream-ordered) */
static int variance_images(RtContext* ctx)
{
    const size_t bytes = (size_t)ctx->localRows * ctx->W * 16;
    if (ctx->dMoments || !bytes) return RT_OK;
    void* m = nullptr;
    void* s = nullptr;
    HIP_TRY(ctx, hipMalloc(&m, bytes));
    const hipError_t e = hipMalloc(&s, bytes);
    if (e != hipSuccess) {
        hipFree(m);
        HIP_TRY(ctx, e);
    }
    ctx->dMoments = m;
    ctx->dSnapshot = s;
    ctx->momentsBytes = bytes;
    hipStream_t st = joined(ctx);
    HIP_TRY(ctx, hipMemsetAsync(m, 0, bytes, st));
    HIP_TRY(ctx, hipMemsetAsync(s, 0, bytes, st));
    return RT_OK;
}

/* what every context call of this header starts with */
static int variance_check_context(RtContext* ctx, const char* call)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    if (ctx->W == 0) return fail(ctx, RT_ERR_STATE, "%s before rt_resize", call);
    return RT_OK;
}

static int variance_update_call(RtContext* ctx, const char* call, bool reset)
{
    int rc = variance_check_context(ctx, call);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RT_FLUSH(ctx);
    if ((rc = variance_images(ctx))) return rc;
    const size_t n = ctx->momentsBytes / 16;
    if (!n) return RT_OK;
    hipStream_t st = joined(ctx);
    if (reset) HIP_TRY(ctx, hipMemsetAsync(ctx->dMoments, 0, ctx->momentsBytes, st));
    HIP_TRY(ctx, rt_vr::enqueue_update(st, accum_target(ctx), ctx->dSnapshot, ctx->dMoments, n, reset ? 1 : 0));
    return RT_OK;
}

int rt_variance_update(RtContext* ctx) { return variance_update_call(ctx, "rt_variance_update", false); }
int rt_variance_reset(RtContext* ctx) { return variance_update_call(ctx, "rt_variance_reset", true); }

int rt_variance_carry(RtContext* ctx, const RtReprojectParams* p, const void* d_prev_aov, const void* d_cur_aov, const void* d_motion, int n_objects)
{
    static const char* call = "rt_variance_carry";
    int rc = variance_check_context(ctx, call);
    if (rc) return rc;
    rt_rp_job job;
    if ((rc = reproject_check_params(ctx, call, p, &job))) return rc;
    if ((rc = check_whole_image(ctx, call, "reprojection", "gather, then rt_reproject_buffers on the moments"))) return rc;
    job.W = ctx->W;
    job.H = ctx->localRows;
    const size_t n = (size_t)job.W * job.H, recBytes = n * sizeof(RtPixelAov);
    const MotionArg mo = {d_motion != nullptr, d_motion, d_motion ? n_objects : 0};
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!d_prev_aov || !d_cur_aov) return fail(ctx, RT_ERR_INVALID_ARG, "%s: %s is null", call, d_prev_aov ? "d_cur_aov" : "d_prev_aov");
    if (n) {
        if ((rc = check_device_range(ctx, call, "d_prev_aov", d_prev_aov, recBytes))) return rc;
        if ((rc = check_device_range(ctx, call, "d_cur_aov", d_cur_aov, recBytes))) return rc;
    } else if (((uintptr_t)d_prev_aov | (uintptr_t)d_cur_aov) & 15) {
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: the records must be 16-byte aligned", call);
    }
    if ((rc = check_motion_table(ctx, call, mo, nullptr, 0))) return rc; /* (what this call writes is the library's own memory) */
    RT_FLUSH(ctx);
    if (!n) return RT_OK;
    if ((rc = variance_images(ctx))) return rc;
    if ((rc = grow_scratch(ctx, &ctx->dDnScratch, &ctx->dnScratchBytes, n * 16))) return rc;
    hipStream_t st = joined(ctx);
    HIP_TRY(ctx, reproject_enqueue(st, job, ctx->dMoments, d_prev_aov, d_cur_aov, mo, ctx->dDnScratch));
    /* over the moments, unless the watchdog of the AOV pass that wrote d_cur_aov fired — rt_reproject_accumulated's commit read the same
     * word and then left the sum alone.  Before any AOV pass of this context there is no such word and nothing to skip for. */
    if (ctx->side[SIDE_AOV].words)
        HIP_TRY(ctx, rt_rp::enqueue_commit(st, ctx->dDnScratch, ctx->dMoments, n, ctx->side[SIDE_AOV].words + kWatchdogWord));
    else
        HIP_TRY(ctx, hipMemcpyAsync(ctx->dMoments, ctx->dDnScratch, n * 16, hipMemcpyDeviceToDevice, st));
    HIP_TRY(ctx, rt_vr::enqueue_update(st, accum_target(ctx), ctx->dSnapshot, ctx->dMoments, n, 1));
    return RT_OK;
}

static int variance_check_moments_call(RtContext* ctx, const char* call, const void* out, size_t bytes)
{
    if (int rc = variance_check_context(ctx, call)) return rc;
    return check_rows_buffer(ctx, call, 16, out, bytes);
}

int rt_variance_read_moments(RtContext* ctx, float* rgba, size_t bytes)
{
    static const char* call = "rt_variance_read_moments";
    int rc = variance_check_moments_call(ctx, call, rgba, bytes);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RT_FLUSH(ctx);
    if ((rc = variance_images(ctx))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(joined(ctx)));
    flush_timer(ctx);
    if ((rc = side_report(ctx, ctx->side[SIDE_AOV], call))) return rc; /* as rt_resolve: a carry behind a pass whose watchdog fired carried nothing */
    if ((rc = check_watchdog(ctx, ctx, call))) return rc;
    if (bytes) HIP_TRY(ctx, hipMemcpy(rgba, ctx->dMoments, bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_variance_moments_to_device(RtContext* ctx, void* d_rgba, size_t bytes)
{
    static const char* call = "rt_variance_moments_to_device";
    int rc = variance_check_moments_call(ctx, call, d_rgba, bytes);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = check_image_out(ctx, call, d_rgba, bytes, nullptr, nullptr))) return rc; /* (against the moments below: they may not exist yet) */
    if (!bytes) return RT_OK;
    RT_FLUSH(ctx);
    if ((rc = variance_images(ctx))) return rc;
    if (ranges_overlap(d_rgba, bytes, ctx->dMoments, bytes)) return fail(ctx, RT_ERR_INVALID_ARG, "%s: d_rgba overlaps the moments", call);
    HIP_TRY(ctx, hipMemcpyAsync(d_rgba, ctx->dMoments, bytes, hipMemcpyDeviceToDevice, joined(ctx)));
    return RT_OK;
}

/* what rt_denoise_variance and rt_denoise_variance_to_device share, as denoise_check_context_call / denoise_enqueue_context_call */
static int variance_check_filter_call(RtContext* ctx, const char* call, const RtVarianceDenoiseParams* p, int aov_frame, const void* out, size_t bytes, rt_vr::Job* job)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    int rc = variance_check_params(ctx, call, p, job);
    if (rc) return rc;
    if (aov_frame < 1) return fail(ctx, RT_ERR_INVALID_ARG, "%s: aov_frame %d < 1 (the first frame after a reset is 1)", call, aov_frame);
    if ((rc = check_renderable(ctx))) return rc;
    if ((rc = check_whole_image(ctx, call, "the filter", "gather, then rt_denoise_variance_buffers"))) return rc;
    if ((rc = check_rows_buffer(ctx, call, 16, out, bytes))) return rc;
    job->W = ctx->W;
    job->H = ctx->localRows;
    return RT_OK;
}

static int variance_enqueue_filter_call(RtContext* ctx, const rt_vr::Job& job, int aov_frame, void* dOut)
{
    const size_t n = (size_t)job.W * job.H;
    int rc;
    if ((rc = variance_images(ctx))) return rc;
    if ((rc = grow_scratch(ctx, &ctx->dDnScratch, &ctx->dnScratchBytes, rt_vr::scratch_bytes(n) + n * 16))) return rc;
    if ((rc = grow_scratch(ctx, &ctx->dDnAov, &ctx->dnAovBytes, n * sizeof(RtPixelAov)))) return rc;
    if ((rc = aov_enqueue(ctx, aov_frame, ctx->dDnAov))) return rc;
    void* resolved = (char*)ctx->dDnScratch + rt_vr::scratch_bytes(n);
    hipStream_t st = joined(ctx);
    HIP_TRY(ctx, rt_rp::enqueue_resolve(st, accum_target(ctx), resolved, n));
    HIP_TRY(ctx, rt_vr::enqueue(st, job, resolved, ctx->dMoments, ctx->dDnAov, dOut, ctx->dDnScratch));
    return RT_OK;
}

int rt_denoise_variance(RtContext* ctx, const RtVarianceDenoiseParams* p, int aov_frame, float* rgba, size_t bytes)
{
    static const char* call = "rt_denoise_variance";
    rt_vr::Job job;
    int rc = variance_check_filter_call(ctx, call, p, aov_frame, rgba, bytes, &job);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RT_FLUSH(ctx);
    if ((rc = side_settle(ctx, ctx->side[SIDE_AOV], call))) return rc;
    if (!bytes) return RT_OK;
    if ((rc = grow_scratch(ctx, &ctx->dDisplay, &ctx->displayBytes, bytes))) return rc;
    if ((rc = variance_enqueue_filter_call(ctx, job, aov_frame, ctx->dDisplay))) return rc;
    return filtered_to_host(ctx, call, rgba, bytes);
}

int rt_denoise_variance_to_device(RtContext* ctx, const RtVarianceDenoiseParams* p, int aov_frame, void* d_rgba, size_t bytes)
{
    static const char* call = "rt_denoise_variance_to_device";
    rt_vr::Job job;
    int rc = variance_check_filter_call(ctx, call, p, aov_frame, d_rgba, bytes, &job);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = check_image_out(ctx, call, d_rgba, bytes, accum_target(ctx), "AccumulatedRender"))) return rc;
    RT_FLUSH(ctx);
    if ((rc = side_settle(ctx, ctx->side[SIDE_AOV], call))) return rc;
    if (!bytes) return RT_OK;
    if ((rc = variance_images(ctx))) return rc;
    if (ranges_overlap(d_rgba, bytes, ctx->dMoments, bytes)) return fail(ctx, RT_ERR_INVALID_ARG, "%s: d_rgba overlaps the moments", call);
    if ((rc = variance_enqueue_filter_call(ctx, job, aov_frame, d_rgba))) return rc;
    ctx->side[SIDE_AOV].unreported = true;
    return RT_OK;
}

} /* extern "C" */
