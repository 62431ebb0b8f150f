/*
 * rt_context.hip — the C ABI of libraytrace_hip.so (include/rt_abi.h): context,
 * render-target ownership, launches.  Every kernel of rt_kernels.h is launched from this
 * unit and from no other; the entry points that launch none are rt_scene_upload.hip's,
 * rt_post.hip's and rt_multi.hip's, over the helpers rt_context.h declares.
 *
 * Replaces the call surface RayComputeManager.cs ("RCM") drives on Unity's
 * ComputeShader/ComputeBuffer objects; see rt_abi.h for the per-function map.
 * There is no CPU fallback: without a HIP device rt_create fails.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>

#include <cmath>
#include <string>
#include <vector>

#include <algorithm>
#include <chrono>

#include "rt_kernels.h"
#include "../../include/rt_cost.h"
#include "../../include/rt_primary.h"
#include "../../include/rt_held_back.h"
#include "../../include/rt_tile_cand.h"
#include "../../include/rt_aov.h"
#include "../../include/rt_motion.h"
#include "../../include/rt_query.h"
#include "../../include/rt_radiance.h"
#include "../../include/rt_nee.h"
#include "../../include/rt_mis.h"

#include "rt_adaptive_launch.h"
#include "rt_query_launch.h"
#include "rt_radiance_launch.h"
#include "rt_nee_launch.h"
#include "rt_mis_launch.h"
#include "rt_light_table.h"
#include "rt_layout.h"
#include "rt_launch_order.h"
#include "rt_launch_plan.h"
#include "rt_scene_prep.h"
#include "rt_primary.h"
#include "rt_tile_cand.h"
#include "rt_context.h"
#define RT_VERSION_STRING "raytrace_hip gfx950 abi=1"

static thread_local char g_err[512] = "";

int fail(RtContext* ctx, int status, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) snprintf(ctx->err, sizeof(ctx->err), "%s", buf);
    snprintf(g_err, sizeof(g_err), "%s", buf);
    return status;
}

/* The main stream, ordered after everything the second render stream has been given.  Every
 * use of the stream other than a render launch goes through here. */
hipStream_t joined(RtContext* ctx)
{
    (void)ctx->order.join(ctx->backend);
    return ctx->stream;
}

static int clear_watchdog(RtContext* ctx)
{
    HIP_TRY(ctx, hipMemsetAsync(ctx->dCounters + kWatchdogWord, 0, sizeof(unsigned long long), joined(ctx)));
    return RT_OK;
}

int watchdog_failure(RtContext* report, const char* call, unsigned long long fired)
{
    return fail(report, RT_ERR_HIP, "%s: a kernel watchdog fired %llu times since the last rt_reset_accumulation / rt_write_accumulated / rt_resize: "
                "walks were cut short or chains dropped, the image is not valid (rt_reset_accumulation clears this)", call, fired);
}

/* Called by every path that hands pixels to a caller, AFTER the synchronise it already performs (8 bytes read back; never on
 * the render path).  `report` receives the message (a multi-context reports through its context 0). */
int check_watchdog(RtContext* ctx, RtContext* report, const char* call)
{
    unsigned long long fired = 0;
    const hipError_t e = hipMemcpy(&fired, ctx->dCounters + kWatchdogWord, sizeof(fired), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(report, RT_ERR_HIP, "%s: reading the watchdog word: %s", call, hipGetErrorString(e));
    return fired ? watchdog_failure(report, call, fired) : RT_OK;
}

/* ---- the watchdog word of a side pass (SidePass): read by the host forms when they return, handed over by the device forms --
 * A device-form pass is reported exactly once, by whichever comes first: rt_synchronize, a host read behind it that says so (rt_resolve,
 * rt_variance_read_moments), or the next call that runs the same pass — side_settle, before that call's own pass clears the word. */
/* After a synchronise of the stream: the pass's own watchdog word (8 bytes read back) */
int side_fired(RtContext* ctx, const SidePass& sp, unsigned long long* fired)
{
    *fired = 0;
    HIP_TRY(ctx, hipMemcpy(fired, sp.words + kWatchdogWord, sizeof(*fired), hipMemcpyDeviceToHost));
    return RT_OK;
}

/* After a synchronise of the stream: the report of a device-form pass that has not been reported yet */
int side_report(RtContext* ctx, SidePass& sp, const char* call)
{
    if (!sp.unreported) return RT_OK;
    sp.unreported = false;
    unsigned long long fired = 0;
    if (int rc = side_fired(ctx, sp, &fired)) return rc;
    if (fired) return fail(ctx, RT_ERR_HIP, "%s: the traversal watchdog fired %llu times in %s: "
                           "walks were cut short, that call's %s are not valid (the context's images are not affected)", call, fired, sp.whose, sp.what);
    return RT_OK;
}

/* a device-form pass still unreported: synchronise and report it before this call's own pass clears the word */
int side_settle(RtContext* ctx, SidePass& sp, const char* call)
{
    if (!sp.unreported) return RT_OK;
    HIP_TRY(ctx, hipStreamSynchronize(joined(ctx)));
    return side_report(ctx, sp, call);
}

int local_rows_for(int H, int stripRows, int partIndex, int partCount)
{
    int rows = 0;
    int nStrips = (H + stripRows - 1) / stripRows;
    for (int s = partIndex; s < nStrips; s += partCount) {
        int r0 = s * stripRows;
        int r1 = r0 + stripRows < H ? r0 + stripRows : H;
        rows += r1 - r0;
    }
    return rows;
}

void flush_timer(RtContext* ctx)
{
    if (ctx->timerState == 2) {
        hipEventSynchronize(ctx->evStop);
        float ms = 0;
        if (hipEventElapsedTime(&ms, ctx->evStart, ctx->evStop) == hipSuccess) ctx->gpuMs += ms;
        ctx->timerState = 0;
    }
}

/* ---- what the entry points behind the render share: targets, scratch, argument checks ------------------------------------------- */
/* The render targets: the caller's (rt_bind_render_targets) or the context's own */
float* accum_target(const RtContext* ctx) { return ctx->boundAccum ? ctx->boundAccum : ctx->ownAccum; }
static float* frame_target(const RtContext* ctx) { return ctx->boundFrame ? ctx->boundFrame : ctx->ownFrame; }
float* image_target(const RtContext* ctx, int use_accumulated) { return use_accumulated ? accum_target(ctx) : frame_target(ctx); }

/* Device scratch that is kept between calls and grows on demand: *buf holds at least `bytes` bytes afterwards */
int grow_scratch(RtContext* ctx, void** buf, size_t* have, size_t bytes)
{
    if (*have >= bytes) return RT_OK;
    HIP_TRY(ctx, hipStreamSynchronize(joined(ctx))); /* work still running on the stream uses the old allocation */
    hipFree(*buf);
    *buf = nullptr;
    *have = 0;
    HIP_TRY(ctx, hipMalloc(buf, bytes));
    *have = bytes;
    return RT_OK;
}

/* `p` is `bytes` bytes of 16-byte aligned device memory of the context's device (kernels write or read through it) */
int check_device_range(RtContext* ctx, const char* call, const char* what, const void* p, size_t bytes)
{
    if (!p) return fail(ctx, RT_ERR_INVALID_ARG, "%s: %s is null", call, what);
    if ((uintptr_t)p & 15) return fail(ctx, RT_ERR_INVALID_ARG, "%s: %s must be 16-byte aligned", call, what);
    hipPointerAttribute_t at;
    void* base = nullptr;
    size_t size = 0;
    if (hipPointerGetAttributes(&at, p) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != ctx->device ||
        hipMemGetAddressRange((hipDeviceptr_t*)&base, &size, (hipDeviceptr_t)p) != hipSuccess || (const char*)p + bytes > (const char*)base + size) {
        (void)hipGetLastError();
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: %s is not %zu bytes of device memory on device %d", call, what, bytes, ctx->device);
    }
    return RT_OK;
}

bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    return (const char*)a < (const char*)b + nb && (const char*)b < (const char*)a + na;
}

/* The caller's buffer for this context's rows: exactly rows x W x perPixel bytes, and a pointer where there are bytes — or always
 * (nullIsError: the reads, the display calls and rt_write_accumulated refuse a null pointer even for a part that owns no rows) */
int check_rows_buffer(RtContext* ctx, const char* call, size_t perPixel, const void* p, size_t bytes, bool nullIsError)
{
    const size_t want = (size_t)ctx->localRows * ctx->W * perPixel;
    if (bytes != want || (!p && (bytes || nullIsError)))
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: need exactly %zu bytes (%d rows x %d x %zu), got %zu%s", call, want, ctx->localRows, ctx->W, perPixel, bytes,
                    p ? "" : " and a null pointer");
    return RT_OK;
}

/* d_rgba of a *_to_device image call, `bytes` bytes: device memory that does not overlap `other` (named `otherName`; nullptr: no such
 * test) — or, without bytes, a pointer that is aligned all the same */
int check_image_out(RtContext* ctx, const char* call, const void* d_rgba, size_t bytes, const void* other, const char* otherName)
{
    if (!bytes) return ((uintptr_t)d_rgba & 15) ? fail(ctx, RT_ERR_INVALID_ARG, "%s: d_rgba must be 16-byte aligned", call) : RT_OK;
    if (int rc = check_device_range(ctx, call, "d_rgba", d_rgba, bytes)) return rc;
    if (other && ranges_overlap(d_rgba, bytes, other, bytes)) return fail(ctx, RT_ERR_INVALID_ARG, "%s: d_rgba overlaps %s", call, otherName);
    return RT_OK;
}

/* The passes that look at a pixel's neighbours need every row.  A context that passes this one owns pixels (part 0 of 1 of an image
 * rt_resize accepted) — unless rt_set_partition stored the whole-image partition over a part without rows and its rt_resize then failed
 * in HIP before it recomputed localRows; for that one case the context calls behind this check still handle zero bytes. */
int check_whole_image(RtContext* ctx, const char* call, const char* who, const char* instead)
{
    if (ctx->partCount > 1)
        return fail(ctx, RT_ERR_STATE, "%s: this context owns part %d of %d of the image; %s needs the whole image (%s)", call, ctx->partIndex, ctx->partCount, who, instead);
    return RT_OK;
}

/* width x height of a *_buffers call.  The limit is the caller's: rt_denoise_buffers admits one pixel less than the reprojection and resolve
 * calls (INT32_MAX / 2 against 1 << 30).  Nothing in rt_denoise.hip's indexing (size_t throughout) asks for that; the limits are kept as they
 * were first written. */
int check_image_size(RtContext* ctx, const char* call, int width, int height, long long maxPixels)
{
    if (width < 1 || height < 1 || (long long)width * height > maxPixels)
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: %d x %d is not an image size (at least 1 x 1, at most 2^30 pixels)", call, width, height);
    return RT_OK;
}

/* Stream-ordered host->device upload: the bytes are copied into a pinned staging slot now and the
 * transfer is enqueued on the (joined) render stream, i.e. after every frame already enqueued and
 * before the next one; the caller's memory is free on return and the host waits for the GPU only when the
 * slot it is about to reuse is still in flight: a host that animates models AND spheres every frame uses 8 of the 24
 * slots per frame, i.e. it blocks once it is three frames ahead of the GPU. */
int stage_upload(RtContext* ctx, void* dst, const void* src, size_t bytes)
{
    if (!bytes) return RT_OK;
    RtContext::Staging& s = ctx->staging[ctx->stagingNext];
    ctx->stagingNext = (ctx->stagingNext + 1) % (int)(sizeof(ctx->staging) / sizeof(ctx->staging[0]));
    if (s.inFlight) {
        HIP_TRY(ctx, hipEventSynchronize(s.done));
        s.inFlight = false;
    }
    if (s.cap < bytes) {
        if (s.host) hipHostFree(s.host);
        s.host = nullptr;
        s.cap = 0;
        size_t cap = bytes < 4096 ? 4096 : bytes + bytes / 2;
        HIP_TRY(ctx, hipHostMalloc(&s.host, cap, hipHostMallocDefault));
        s.cap = cap;
    }
    if (!s.done) HIP_TRY(ctx, hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    memcpy(s.host, src, bytes);
    hipStream_t st = joined(ctx);
    HIP_TRY(ctx, hipMemcpyAsync(dst, s.host, bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipEventRecord(s.done, st));
    s.inFlight = true;
    ctx->updateUploads++;
    return RT_OK;
}

static int launch_frames(RtContext* ctx, int frame0, int nFrames);
static bool gpu_idle(RtContext* ctx);

/* Launch the frames rt_render_frame held back.  Called first thing by every entry point that reads or changes
 * what those frames depend on, or that hands results to the host. */
int flush_pending(RtContext* ctx)
{
    if (!ctx || ctx->pending == 0) return RT_OK;
    const int n = ctx->pending;
    ctx->pending = 0;
    hipSetDevice(ctx->device);
    ctx->lastLaunched = 0;
    const int rc = launch_frames(ctx, ctx->frame - n, n);
    if (rc != RT_OK) ctx->frame -= n - ctx->lastLaunched; /* the frames that never ran: the frame counter says so (the caller may retry them) */
    return rc;
}

extern "C" {

const char* rt_version(void) { return RT_VERSION_STRING; }

const char* rt_last_error(const RtContext* ctx) { return ctx ? ctx->err : g_err; }

int rt_create(int device_id, RtContext** out)
{
    if (!out) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_create: out is null");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, RT_ERR_NO_DEVICE, "rt_create: no HIP device (%s); libraytrace_hip has no CPU fallback",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device_id < 0 || device_id >= n) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_create: device %d out of range [0,%d)", device_id, n);
    RtContext* ctx = new RtContext();
    ctx->device = device_id;
    ctx->backend.ctx = ctx;
    auto init = [&]() -> int {
        HIP_TRY(ctx, hipSetDevice(device_id));
        hipDeviceProp_t prop;
        HIP_TRY(ctx, hipGetDeviceProperties(&prop, device_id));
        ctx->numCUs = prop.multiProcessorCount;
        HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->ownStream, hipStreamNonBlocking));
        ctx->stream = ctx->ownStream;
        HIP_TRY(ctx, hipMalloc(&ctx->dCounters, sizeof(unsigned long long) * RT_COUNTER_SLOTS * RT_COUNTER_FIELDS));
        /* Every fill goes through the context's own stream: hipMemset on the null stream may return before the fill has
         * run, and the render streams are non-blocking, i.e. NOT ordered after the null stream — a late fill would then
         * wipe what the first kernels have already counted (seen with two processes sharing one GPU: 4 % of a launch's
         * segments lost once in 20 runs). */
        HIP_TRY(ctx, hipMemsetAsync(ctx->dCounters, 0, sizeof(unsigned long long) * RT_COUNTER_SLOTS * RT_COUNTER_FIELDS, ctx->ownStream));
        HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->sideStream, hipStreamNonBlocking)); /* (a higher priority for it measured no different) */
        HIP_TRY(ctx, hipMalloc(&ctx->dTileQueue, 2 * sizeof(unsigned long long)));
        HIP_TRY(ctx, hipMemsetAsync(ctx->dTileQueue, 0, 2 * sizeof(unsigned long long), ctx->ownStream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->ownStream));
        HIP_TRY(ctx, hipEventCreate(&ctx->evStart));
        HIP_TRY(ctx, hipEventCreate(&ctx->evStop));
        for (hipEvent_t& ev : ctx->backend.ev) HIP_TRY(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        return RT_OK;
    };
    if (int rc = init()) { /* the message stays readable through rt_last_error(NULL) */
        rt_destroy(ctx);
        return rc;
    }
    memset(&ctx->params, 0, sizeof(ctx->params));
    if (const char* g = getenv("RT_GRID")) ctx->gridOverride = atoi(g); /* tuning hook */
    if (const char* g = getenv("RT_POOL_MIN_ITEMS")) ctx->poolMinItems = atoi(g);
    if (const char* g = getenv("RT_PRIMARY")) ctx->primaryOn = atoi(g) != 0;
    if (const char* g = getenv("RT_TILE_CAND")) ctx->tileCandOn = atoi(g) != 0;
    if (const char* g = getenv("RT_TILE_TRI")) ctx->tileTriOn = atoi(g) != 0;
    if (const char* g = getenv("RT_SKY_SUN")) ctx->skySunOn = atoi(g) != 0;
    if (const char* g = getenv("RT_POOL_FAULT")) { if (atoi(g)) ctx->poolSpinLimit = 64u | 0x80000000u; }
    if (getenv("RT_VERBOSE")) ctx->verbose = true;
    if (const char* f = getenv("RT_FUSE_FRAMES")) ctx->fuseFrames = atoi(f) != 0;
    if (const char* l = getenv("RT_LPT")) ctx->order.lpt = atoi(l) != 0;
    if (const char* t = getenv("RT_TWO_STREAMS")) ctx->twoStreams = atoi(t) != 0;
    if (const char* c = getenv("RT_COALESCE")) ctx->coalesce = atoi(c) != 0;
    if (const char* hb = getenv("RT_HOLD_BACK")) ctx->holdBack = atoi(hb) != 0; /* test hook */
    if (const char* fg = getenv("RT_FRAME_GROUP")) ctx->frameGroupOverride = atoi(fg);
    if (const char* al = getenv("RT_ALTERNATE")) ctx->order.alternate = ctx->alternateWanted = atoi(al) != 0;
    ctx->order.set_two_streams(ctx->twoStreams && ctx->sideStream);
    if (const char* fc = getenv("RT_FUSE_CAP"))
        if (const int cap = rt_plan::pinned_fuse_cap(atoi(fc))) { ctx->fuseCap = cap; ctx->fuseCapPinned = true; }
    *out = ctx;
    return RT_OK;
}

void rt_destroy(RtContext* ctx)
{
    if (!ctx) return;
    hipSetDevice(ctx->device);
    flush_pending(ctx);
    if (ctx->sideStream) hipStreamSynchronize(ctx->sideStream);
    hipStreamSynchronize(ctx->stream);
    free_scene(ctx);
    hipFree(ctx->ownFrame);
    hipFree(ctx->ownAccum);
    hipFree(ctx->dCounters);
    hipFree(ctx->dTileQueue);
    hipFree(ctx->dTileCost);
    hipFree(ctx->dTileOrder[0]);
    hipFree(ctx->dTileOrder[1]);
    hipFree(ctx->dTileKey);
    hipFree(ctx->dTileCand[0]);
    hipFree(ctx->dTileCand[1]);
    hipFree(ctx->dDisplay);
    hipFree(ctx->dAovOut);
    hipFree(ctx->dRays);
    hipFree(ctx->dRayOut);
    for (SidePass& sp : ctx->side) hipFree(sp.words);
    hipFree(ctx->dLightTable);
    hipFree(ctx->dLightMap);
    hipFree(ctx->dDnScratch);
    hipFree(ctx->dDnAov);
    hipFree(ctx->dMoments);
    hipFree(ctx->dSnapshot);
    hipFree(ctx->dAdTileError);
    hipFree(ctx->dAdTiles);
    hipFree(ctx->dAdCounts);
    hipFree(ctx->dAdQueue);
    hipFree(ctx->dStaging[0]);
    hipFree(ctx->dStaging[1]);
    hipFree(ctx->dPxCold);
    for (auto& pr : ctx->tuner.probe) {
        if (pr.start) hipEventDestroy(pr.start);
        if (pr.stop) hipEventDestroy(pr.stop);
    }
    for (RtContext::Staging& st : ctx->staging) {
        if (st.host) hipHostFree(st.host);
        if (st.done) hipEventDestroy(st.done);
    }
    for (auto& fp : ctx->fuseProbe) { if (fp.start) hipEventDestroy(fp.start); if (fp.stop) hipEventDestroy(fp.stop); }
    if (ctx->evStart) hipEventDestroy(ctx->evStart);
    if (ctx->evStop) hipEventDestroy(ctx->evStop);
    for (hipEvent_t ev : ctx->backend.ev) if (ev) hipEventDestroy(ev);
    if (ctx->sideStream) hipStreamDestroy(ctx->sideStream);
    if (ctx->ownStream) hipStreamDestroy(ctx->ownStream);
    delete ctx;
}

int rt_set_stream(RtContext* ctx, void* hip_stream)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    RT_FLUSH(ctx);
    hipStreamSynchronize(joined(ctx));
    flush_timer(ctx);
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->ownStream;
    ctx->order.set_two_streams(ctx->twoStreams && ctx->stream == ctx->ownStream); /* a caller's stream: its order is the contract, one stream */
    return RT_OK;
}

int rt_set_partition(RtContext* ctx, int strip_rows, int part_index, int part_count)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    RT_FLUSH(ctx);
    if (strip_rows <= 0 || strip_rows % 8 || part_count <= 0 || part_index < 0 || part_index >= part_count)
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_set_partition: strip_rows must be a positive multiple of 8, 0 <= index < count");
    ctx->stripRows = strip_rows;
    ctx->partIndex = part_index;
    ctx->partCount = part_count;
    if (ctx->W > 0) return rt_resize(ctx, ctx->W, ctx->H);
    return RT_OK;
}

int rt_resize(RtContext* ctx, int width, int height)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    RT_FLUSH(ctx);
    if (width <= 0 || height <= 0) return fail(ctx, RT_ERR_INVALID_ARG, "rt_resize: %dx%d", width, height);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(joined(ctx)));
    ctx->W = width;
    ctx->H = height;
    ctx->localRows = local_rows_for(height, ctx->stripRows, ctx->partIndex, ctx->partCount);
    size_t bytes = (size_t)ctx->localRows * width * 16;
    if (bytes != ctx->ownBytes) {
        hipFree(ctx->ownFrame); ctx->ownFrame = nullptr;
        hipFree(ctx->ownAccum); ctx->ownAccum = nullptr;
        ctx->ownBytes = 0;
        if (bytes) {
            HIP_TRY(ctx, hipMalloc(&ctx->ownFrame, bytes));
            HIP_TRY(ctx, hipMalloc(&ctx->ownAccum, bytes));
            ctx->ownBytes = bytes;
        }
    }
    if (bytes) {
        HIP_TRY(ctx, hipMemsetAsync(ctx->ownFrame, 0, bytes, joined(ctx)));
        HIP_TRY(ctx, hipMemsetAsync(ctx->ownAccum, 0, bytes, joined(ctx)));
    }
    if (int rc = clear_watchdog(ctx)) return rc; /* new targets: nothing rendered into them yet */
    ctx->boundFrame = ctx->boundAccum = nullptr;
    hipFree(ctx->dMoments); ctx->dMoments = nullptr; /* (the stream is idle: synchronised above) */
    hipFree(ctx->dSnapshot); ctx->dSnapshot = nullptr;
    ctx->momentsBytes = 0;
    hipFree(ctx->dAdTileError); ctx->dAdTileError = nullptr; /* the tile list and the tile errors belong to the old geometry */
    hipFree(ctx->dAdTiles); ctx->dAdTiles = nullptr;
    ctx->adTilesTotal = -1;
    ctx->adHaveList = ctx->adHaveErrors = false;
    ctx->adTilesActive = ctx->adPixelsActive = 0;
    ctx->orderTiles = 0; /* tile costs belong to the old geometry */
    for (int i = 0; i < 2; i++)
        if (ctx->dStaging[i]) {
            hipFree(ctx->dStaging[i]); /* sized for the old image: re-made by the next fused launch */
            ctx->dStaging[i] = nullptr;
            ctx->stagingBytes[i] = 0;
        }
    ctx->stagingUnavailable = false;
    ctx->order.alternate = ctx->alternateWanted; /* (a slab that did not fit the old image may fit this one: ADVICE r4) */
    if (!ctx->fuseCapPinned) ctx->fuseCap = RT_FUSE_MIN; /* frame times of the old geometry say nothing */
    for (auto& fp : ctx->fuseProbe) fp.live = false;
    ctx->fuseLast = -1;
    return RT_OK;
}

int rt_local_rows(const RtContext* ctx) { return ctx ? ctx->localRows : RT_ERR_INVALID_ARG; }

int rt_local_to_global_row(const RtContext* ctx, int local_row)
{
    if (!ctx || local_row < 0 || local_row >= ctx->localRows) return RT_ERR_INVALID_ARG;
    int ls = local_row / ctx->stripRows;
    return (ls * ctx->partCount + ctx->partIndex) * ctx->stripRows + (local_row - ls * ctx->stripRows);
}

int rt_bind_render_targets(RtContext* ctx, void* d_frame, void* d_accum)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    RT_FLUSH(ctx);
    if (((uintptr_t)d_frame | (uintptr_t)d_accum) & 15) return fail(ctx, RT_ERR_INVALID_ARG, "render targets must be 16-byte aligned");
    HIP_TRY(ctx, hipStreamSynchronize(joined(ctx)));
    ctx->boundFrame = (float*)d_frame;
    ctx->boundAccum = (float*)d_accum;
    return RT_OK;
}

int rt_get_render_targets(RtContext* ctx, void** d_frame, void** d_accum)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    /* a host that reads the targets after its own device synchronise must find every requested frame at least launched */
    RT_FLUSH(ctx);
    if (d_frame) *d_frame = frame_target(ctx);
    if (d_accum) *d_accum = accum_target(ctx);
    return RT_OK;
}

int rt_set_params(RtContext* ctx, const RtParams* p)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    if (!p) return fail(ctx, RT_ERR_INVALID_ARG, "rt_set_params: null params");
    if (p->abi_version != RT_ABI_VERSION || p->struct_size != sizeof(RtParams))
        return fail(ctx, RT_ERR_ABI_MISMATCH, "rt_set_params: abi_version %u / struct_size %u, library has %u / %zu", p->abi_version,
                    p->struct_size, (unsigned)RT_ABI_VERSION, sizeof(RtParams));
    if (ctx->haveParams && p->frame == ctx->frame) { /* SetShaderParams runs every frame (RCM:122): usually nothing but Frame moved, and it moved to where the context already is */
        RtParams a = *p, b = ctx->params;
        a.frame = b.frame = 0;
        if (memcmp(&a, &b, sizeof(RtParams)) == 0) return RT_OK;
    }
    RT_FLUSH(ctx);
    ctx->params = *p;
    ctx->frame = p->frame;
    ctx->haveParams = true;
    return RT_OK;
}

int rt_reset_accumulation(RtContext* ctx)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    RT_FLUSH(ctx);
    if (ctx->W == 0) return fail(ctx, RT_ERR_STATE, "rt_reset_accumulation before rt_resize");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    size_t n = (size_t)ctx->localRows * ctx->W;
    if (n) {
        int blocks = (int)((n + 255) / 256);
        if (blocks > 2048) blocks = 2048;
        hipLaunchKernelGGL(rtk::rt_reset_kernel, dim3(blocks), dim3(256), 0, joined(ctx), (float4*)accum_target(ctx), n);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (int rc = clear_watchdog(ctx)) return rc;
    ctx->frame = 1; /* RCM:71 */
    return RT_OK;
}

/* withTable: the launch is one of the trace kernels' (launch_frames, adaptive_launch) — the only readers of the table of per-launch
 * origin constants (rt_primary.h); every other launch carries it switched off and pays nothing for it.
 * traceBody: the launch runs trace_body (launch_frames, adaptive_launch, rt_render_cost), whose every ray direction is rt_normalize's
 * result: it may carry RT_USESKY_SUN_UNSEEN (rt_sky.h).  The side passes (AOV, query, radiance, NEE) must NOT: their first segment
 * carries the caller's direction, unnormalised — dir = (0, -1e30, 0) is NaN (inf * 0) in the full GetEnvironmentLight and 0.35 without
 * the sun's addend — so their fill leaves the bit clear, and their kernels do not even test it. */
static void fill_args(RtContext* ctx, int frame0, int nFrames, KArgs& a, bool withTable = false, bool traceBody = false)
{
    memset(&a, 0, sizeof(a));
    a.spheres = ctx->dSpheres;
    a.sphereQuick = ctx->dSpheres + 4 * (size_t)ctx->nSpheres;
    a.sphereBound = ctx->sphereBound;
    a.materials = ctx->dMaterials;
    a.models = ctx->dModels;
    a.pairs = reinterpret_cast<const DPair*>(ctx->dPairs);
    a.tris = reinterpret_cast<const DTri*>(ctx->arenaLayout ? ctx->dPairs : ctx->dTris);
    a.norms = reinterpret_cast<const DTriN*>(ctx->dNorms);
    a.bigLeaves = ctx->dBigLeaves;
    a.filters = ctx->dFilters;
    a.filterPairs = reinterpret_cast<const float*>(ctx->dFilters + ctx->nModels);
    a.chunks = ctx->dChunks;
    a.nChunks = ctx->nChunks;
    a.nFiltered = ctx->nFiltered;
    a.extWords = ctx->extWords;
    a.filterMaxOrigin = ctx->filterMaxOrigin;
    a.nSpheres = ctx->nSpheres;
    a.nModels = ctx->nModels;
    a.frameRender = frame_target(ctx);
    a.accumulated = accum_target(ctx);
    a.W = (uint32_t)ctx->W;
    a.H = (uint32_t)ctx->H;
    a.localRows = ctx->localRows;
    a.stripRows = ctx->stripRows;
    a.partIndex = ctx->partIndex;
    a.partCount = ctx->partCount;
    a.tilesX = (ctx->W + 7) / 8;
    a.tilesY = (ctx->localRows + 7) / 8;
    const RtParams& p = ctx->params;
    a.maxBounce = p.maxBounceCount;
    a.spp = p.numRaysPerPixel;
    a.frame0 = frame0;
    a.nFrames = nFrames;
    a.seed = p.renderSeed;
    a.useSky = p.useSky ? RT_USESKY_ON : 0;
    if (traceBody && ctx->skySunOn && sky_sun_unseen(p)) a.useSky |= RT_USESKY_SUN_UNSEEN; /* decided per launch, from this launch's uniforms */
    a.accumulate = p.accumulate;
    a.defocus = p.defocusStrength;
    a.diverge = p.divergeStrength;
    a.sunFocus = p.sunFocus;
    a.sunIntensity = p.sunIntensity;
    memcpy(a.sunColour, p.sunColour, 12);
    memcpy(a.dirToSun, p.dirToSun, 12);
    memcpy(a.viewParams, p.viewParams, 12);
    memcpy(a.cam, p.camLocalToWorld, 64);
    a.rcpWm1 = rt_rcp((float)a.W - 1.0f);
    a.rcpHm1 = rt_rcp((float)a.H - 1.0f);
    a.rcpW = rt_rcp((float)a.W);
    a.rcpSpp = rt_rcp((float)a.spp);
    {
        /* x + (+-0) == x bit for bit unless x is -0 (then the sign of the sum follows the random jitter's sign):
         * the kernel may skip the defocus jitter's sin/cos/sqrt when no component of the camera origin — computed
         * here with the kernel's own rt_mul_point — is a negative zero */
        bool fin = true;
        for (int k = 0; k < 16; k++) fin = fin && std::isfinite(a.cam[k]);
        const rt_f3 o = primary_cam_origin(a.cam);
        const bool noNegZero = rt_f2u(o.x) != 0x80000000u && rt_f2u(o.y) != 0x80000000u && rt_f2u(o.z) != 0x80000000u;
        a.raygenNoDefocus = (a.defocus == 0.0f && fin && noNegZero && std::isfinite(a.rcpW)) ? 1 : 0;
        /* the same value is the FLAT kernels' camera-ray origin (raygen) and the origin of the table of per-launch constants
         * (rt_primary.h), rebuilt here for every launch from the host mirrors of what the stream holds at that launch: the
         * update calls flush the frames held back before they change a mirror */
        const bool allowed = withTable && ctx->haveScene &&
                             primary_allowed(ctx->primaryOn, a.raygenNoDefocus != 0, ctx->flatScene, ctx->nSpheres, ctx->nModels, ctx->primaryTris);
        std::vector<float> sph;
        DModel dm[RT_PRIMARY_MAX_MODELS];
        if (allowed) {
            float bound; /* (== ctx->sphereBound: the same function over the same mirror) */
            pack_spheres(ctx->hSpheres.data(), ctx->nSpheres, sph, &bound);
            for (int i = 0; i < ctx->nModels; i++) pack_model(ctx->hModels[i], ctx->hRootCodes[i], ctx->hTriBase[i], dm[i]);
        }
        primary_fill(a.primary, allowed, o, sph.data(), ctx->nSpheres, ctx->sphereBound, dm, ctx->nModels, ctx->primaryTris);
        if (withTable) {
            ctx->lastPrimaryOn = a.primary.on;
            /* the per-tile sphere candidates ride on the table: the same launches, the same caps, the same mirror of the spheres */
            ctx->lastTileCand = 0;
            ctx->lastTileTri = 0;
            ctx->tileCandWanted = ctx->tileCandOn && a.primary.on != 0;
            if (ctx->tileCandWanted) {
                TileCandKey& k = ctx->tileCandWant;
                tile_cand_key_init(k);
                memcpy(k.cam, a.cam, sizeof(k.cam));
                memcpy(k.viewParams, a.viewParams, sizeof(k.viewParams));
                k.rcpWm1 = a.rcpWm1; k.rcpHm1 = a.rcpHm1; k.rcpW = a.rcpW; k.diverge = a.diverge;
                k.camOrigin[0] = o.x; k.camOrigin[1] = o.y; k.camOrigin[2] = o.z;
                k.W = (int32_t)a.W; k.H = (int32_t)a.H;
                k.tilesX = a.tilesX; k.tiles = a.tilesX * a.tilesY;
                k.stripRows = a.stripRows; k.partIndex = a.partIndex; k.partCount = a.partCount;
                k.nSpheres = ctx->nSpheres;
                memcpy(k.sph, sph.data(), sizeof(float) * 4 * (size_t)ctx->nSpheres); /* pack_spheres' exact records; primary.on: at most 32 */
                /* the triangle half: what traverse_flat and tri_test read in these waves — the packed w2l rows, the table's lpos and the
                 * laid-out local records (primary.on: within RT_PRIMARY_MAX_MODELS / RT_PRIMARY_MAX_TRIS, the caps of the mask) */
                const PrimaryTris& pt = ctx->primaryTris;
                k.triOn = ctx->tileTriOn ? 1 : 0;
                if (k.triOn) {
                    k.nTriModels = ctx->nModels;
                    int t = 0;
                    for (int m = 0; m < ctx->nModels; m++) {
                        k.triCount[m] = pt.count[m];
                        memcpy(k.w2l[m], dm[m].w2l, sizeof(k.w2l[m]));
                        memcpy(k.lpos[m], a.primary.lpos[m], sizeof(k.lpos[m]));
                        for (int i = 0; i < pt.count[m]; i++, t++) {
                            memcpy(&k.tri[t][0], pt.a[t], 12); memcpy(&k.tri[t][3], pt.ab[t], 12);
                            memcpy(&k.tri[t][6], pt.ac[t], 12); memcpy(&k.tri[t][9], pt.face[t], 12);
                        }
                    }
                }
            }
        }
    }
    a.counters = ctx->dCounters;
    a.travLimit = ctx->travLimit;
    a.poolSpinLimit = ctx->poolSpinLimit;
    a.wavesPerGroup = 1; /* (choose_variant decides the workgroup shape of the trace kernels; the debug hooks run single waves without a cache) */
}

} /* extern "C" */

/* =====================================================================================================================
 * The launch path.  rt_render_frame / rt_render_frames / flush_pending end in launch_frames(ctx, frame0, nFrames):
 *     choose_variant    which kernel instantiation, how much LDS, how many workgroups the chip keeps resident (LaunchPlan)
 *     prepare_*         the buffers a launch needs — pixel records, tile order, staging slab; may synchronise (rarely)
 *     LaunchOrder       place: which stream(s), how many parts, whether the tile order is re-sorted (rt_launch_order.h);
 *                       run: the sort, trace and accumulate kernels through HipOrder, with the events that order the two streams
 * Every size on this path — workgroup shape, LDS, grid, items, tile-queue positions, slab frames, frames per fused launch, the tuner's
 * choice — is decided by rt_launch_plan.h; what is left here is the HIP work around it.
 * Dispatch semantics kept: RayComputeManager.cs:84-95 (one RayTrace dispatch per frame, Frame counts the accumulated frames).
 * ===================================================================================================================== */
struct LaunchPlan {
    void (*kern)(const KArgs) = nullptr;     /* a launch that renders a whole frame or a batch of frames */
    void (*kernHalf)(const KArgs) = nullptr; /* the same code under a second name: the two halves of a two-part frame (rt_kernels.h) */
    rt_plan::LaunchShape shape;  /* workgroup shape, LDS, variant = slot of the occupancy cache */
    long long resident = 0;      /* workgroups the chip keeps resident */
};

/* ---- choose variant: kernel instantiation, LDS, resident workgroups */
/* the trace kernel's instantiations <STATS, FLAT, MANY, HOT>, indexed by rt_plan::LaunchShape::variant = stats + 2 flat + 4 many + 6 hot */
#define RT_TRACE_VARIANT(STATS, FLAT, MANY, HOT) {rtk::rt_trace_kernel<STATS, FLAT, MANY, HOT>, rtk::rt_trace_half_kernel<STATS, FLAT, MANY, HOT>}
static const struct { void (*kern)(const KArgs); void (*kernHalf)(const KArgs); } kTraceVariants[] = {
    RT_TRACE_VARIANT(false, false, false, false), RT_TRACE_VARIANT(true, false, false, false), /* 0, 1: BVH, single waves */
    RT_TRACE_VARIANT(false, true, false, false),  RT_TRACE_VARIANT(true, true, false, false),  /* 2, 3: FLAT, single waves */
    RT_TRACE_VARIANT(false, false, true, false),  RT_TRACE_VARIANT(true, false, true, false),  /* 4, 5: BVH > 64 models, single waves */
    RT_TRACE_VARIANT(false, false, false, true),  RT_TRACE_VARIANT(true, false, false, true),  /* 6, 7: BVH, top-of-tree cache */
    RT_TRACE_VARIANT(false, true, false, true),   RT_TRACE_VARIANT(true, true, false, true),   /* 8, 9: FLAT, chain pool */
    RT_TRACE_VARIANT(false, false, true, true),   RT_TRACE_VARIANT(true, false, true, true),   /* 10, 11: BVH > 64 models, top-of-tree cache */
};
#undef RT_TRACE_VARIANT
static_assert(sizeof(kTraceVariants) / sizeof(kTraceVariants[0]) == RT_TRACE_VARIANTS, "one trace kernel per variant slot");
static_assert(RT_TRACE_VARIANTS <= sizeof(RtContext::occPerCU) / sizeof(int), "the occupancy cache has a slot per variant");

static int choose_variant(RtContext* ctx, KArgs& a, LaunchPlan& plan)
{
    rt_plan::SceneShape sc;
    sc.flat = ctx->flatScene;
    sc.stats = ctx->stats;
    sc.stackEntries = ctx->stackEntries;
    sc.extWords = ctx->extWords;
    sc.nChunks = ctx->nChunks;
    sc.hotUnits = ctx->hotUnits;
    sc.wavesPerGroup = ctx->wavesPerGroup;
    sc.poolCells = ctx->poolCells;
    sc.poolWaves = ctx->poolWaves;
    sc.poolMinItems = ctx->poolMinItems;
    sc.numCUs = ctx->numCUs;
    const rt_plan::LaunchShape& sh = plan.shape = rt_plan::launch_shape(sc, (long long)a.tilesX * a.tilesY, a.nFrames);
    plan.kern = kTraceVariants[sh.variant].kern;
    plan.kernHalf = kTraceVariants[sh.variant].kernHalf;
    a.wavesPerGroup = sh.wavesPerGroup;
    a.hotUnits = (int32_t)sh.hotUnits;
    a.poolCells = sh.poolCells;
    a.waveLdsDwords = sh.waveLdsDwords;
    a.stackEntries = ctx->stackEntries;
    if (ctx->occBytes[sh.variant] != sh.ldsBytes + 1) { /* occupancy query cached per (variant, LDS bytes) */
        int perCU = 0;
        if (sh.ldsBytes > 48 * 1024) { /* more dynamic LDS than the default limit of a launch */
            HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(plan.kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh.ldsBytes));
            HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(plan.kernHalf), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh.ldsBytes));
        }
        HIP_TRY(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, plan.kern, sh.blockThreads, sh.ldsBytes));
        ctx->occPerCU[sh.variant] = perCU > 0 ? perCU : 1;
        ctx->occBytes[sh.variant] = sh.ldsBytes + 1;
        if (getenv("RT_DEBUG_LAUNCH"))
            fprintf(stderr, "[rt] kernel variant %d: %d stack entries, %zu B of LDS per workgroup of %d threads (%u B of it the top-of-tree cache: %u records), %d workgroups per CU\n",
                    sh.variant, ctx->stackEntries, sh.ldsBytes, sh.blockThreads, sh.hotUnits * 16u, sh.hotUnits / 4u, perCU);
    }
    plan.resident = (long long)ctx->occPerCU[sh.variant] * ctx->numCUs;
    return RT_OK;
}

/* ---- prepare buffers: the resident waves' pixel records */
static int prepare_records(RtContext* ctx, const LaunchPlan& plan)
{
    const long long waves = rt_plan::record_waves(plan.resident, plan.shape.wavesPerGroup, ctx->gridOverride);
    if (ctx->pxColdWaves < waves) { /* kernels in flight use the old block: freed after a synchronise, not now */
        HIP_TRY(ctx, hipStreamSynchronize(joined(ctx)));
        hipFree(ctx->dPxCold); ctx->dPxCold = nullptr; ctx->pxColdWaves = 0;
        HIP_TRY(ctx, hipMalloc(&ctx->dPxCold, (size_t)2 * waves * RT_COLD_STRIDE_BYTES));
        ctx->pxColdWaves = waves;
    }
    return RT_OK;
}

/* ---- prepare buffers: longest-chain-first queue order, learnt from the frames already rendered at this size.  Re-sorted once 1, 2, 4, 8,
 * ... frames have been recorded; the sort runs on the stream of the launch that first uses it, writes the order buffer that no running
 * kernel reads, works on its own snapshot of the costs (running kernels keep raising them) — it never joins the two streams (a join in the
 * middle of back-to-back launches serialises the next launch behind the drain of the previous one; round 4). */
static int prepare_tile_order(RtContext* ctx, KArgs& a, int tiles)
{
    if (!ctx->order.lpt) return RT_OK;
    if (ctx->orderTiles != tiles) {
        HIP_TRY(ctx, hipStreamSynchronize(joined(ctx)));
        hipFree(ctx->dTileCost); ctx->dTileCost = nullptr;
        hipFree(ctx->dTileOrder[0]); hipFree(ctx->dTileOrder[1]); ctx->dTileOrder[0] = ctx->dTileOrder[1] = nullptr;
        hipFree(ctx->dTileKey); ctx->dTileKey = nullptr;
        HIP_TRY(ctx, hipMalloc(&ctx->dTileCost, sizeof(uint32_t) * tiles));
        HIP_TRY(ctx, hipMalloc(&ctx->dTileOrder[0], sizeof(uint32_t) * tiles));
        HIP_TRY(ctx, hipMalloc(&ctx->dTileOrder[1], sizeof(uint32_t) * tiles));
        HIP_TRY(ctx, hipMalloc(&ctx->dTileKey, sizeof(uint32_t) * tiles));
        HIP_TRY(ctx, hipMemsetAsync(ctx->dTileCost, 0, sizeof(uint32_t) * tiles, joined(ctx)));
        ctx->orderTiles = tiles;
        ctx->order.forget_order();
    }
    a.tileCost = ctx->dTileCost;
    return RT_OK;
}

/* ---- prepare buffers: the two streams' tables of per-tile sphere candidates (rt_tile_cand.h), when the launch may read one.  A launch
 * that finds no memory for them runs with the per-ray pre-test: results do not depend on the table. */
static int prepare_tile_cand(RtContext* ctx, int tiles)
{
    if (!ctx->tileCandWanted || ctx->tileCandTiles == tiles) return RT_OK;
    HIP_TRY(ctx, hipStreamSynchronize(joined(ctx))); /* kernels in flight read the old tables */
    ctx->tileCandTiles = 0;
    for (int s = 0; s < 2; s++) {
        hipFree(ctx->dTileCand[s]); ctx->dTileCand[s] = nullptr;
        ctx->tileCandValid[s] = false;
    }
    for (int s = 0; s < 2; s++)
        if (hipMalloc(&ctx->dTileCand[s], 2 * sizeof(uint32_t) * (size_t)tiles) != hipSuccess) { /* (sphere mask, triangle mask) per tile */
            (void)hipGetLastError();
            ctx->dTileCand[s] = nullptr;
            ctx->tileCandWanted = false;
            return RT_OK;
        }
    ctx->tileCandTiles = tiles;
    return RT_OK;
}

/* ---- prepare buffers: the staging slab of a fused launch ([frame][pixel] colours awaiting rt_accumulate_kernel), one per stream so that
 * consecutive fused launches can alternate between the streams.  Returns 1 when the launch cannot be staged on this lane (the caller
 * falls back), 0 when a.staging is set. */
static_assert(sizeof(float4) == RT_STAGED_PIXEL_BYTES, "a staged colour is one float4");
static int prepare_staging(RtContext* ctx, KArgs& a, int nFrames, size_t nPix, int lane, bool split, bool* unavailable)
{
    *unavailable = false;
    const size_t need = (size_t)nFrames * nPix * RT_STAGED_PIXEL_BYTES;
    if (!ctx->stagingUnavailable && ctx->stagingBytes[lane] < need) {
        HIP_TRY(ctx, hipStreamSynchronize(joined(ctx)));
        /* both slabs are made by the first fused launch (a warm-up launch then pays for both: an allocation of this size takes
         * milliseconds); sized for the largest batch this context forms; if memory is short, for this batch */
        for (int sl = 0; sl < (split && ctx->order.alternate ? 2 : 1); sl++) {
            const int b = sl == 0 ? lane : 1 - lane;
            if (ctx->stagingBytes[b] >= need) continue;
            hipFree(ctx->dStaging[b]);
            ctx->dStaging[b] = nullptr;
            ctx->stagingBytes[b] = 0;
            /* room for the largest batch this context will ever form, so that a growing cap never re-makes a slab in the middle of a
             * render (rt_plan::slab_frames; the cap is held to what the slabs hold: rt_plan::fuse_cap) */
            /* (sized ONCE, at the first fused launch, on purpose: growing a slab later costs a synchronise + an allocation of this size in the
             * middle of a progressive render.  BVH scenes never batch more than RT_FUSE_MIN frames: a host that runs many contexts of such
             * scenes lowers the budget with RT_FUSE_SLAB_MB — ADVICE r5) */
            size_t slabBudget = RT_FUSE_SLAB_BYTES;
            if (const char* e = getenv("RT_FUSE_SLAB_MB")) { const long long mb = atoll(e); if (mb > 0) slabBudget = (size_t)mb << 20; }
            const size_t cap = rt_plan::slab_frames(nPix, slabBudget, nFrames) * nPix * RT_STAGED_PIXEL_BYTES;
            size_t got = cap;
            if (hipMalloc(&ctx->dStaging[b], cap) != hipSuccess) {
                (void)hipGetLastError();
                ctx->dStaging[b] = nullptr;
                got = need;
                if (hipMalloc(&ctx->dStaging[b], need) != hipSuccess) {
                    (void)hipGetLastError();
                    ctx->dStaging[b] = nullptr;
                    got = 0;
                }
            }
            ctx->stagingBytes[b] = got;
            if (got < need && b != lane) ctx->order.alternate = false; /* no room for the second slab: fused launches stay on one stream (until rt_resize) */
        }
    }
    if (ctx->stagingUnavailable || ctx->stagingBytes[lane] < need) {
        *unavailable = true;
        return RT_OK;
    }
    a.staging = ctx->dStaging[lane];
    a.stagingStride = (uint32_t)nPix;
    return RT_OK;
}

/* ---- launch tuner (suspension threshold 3/8 or 4/8) and the frames-per-launch budget: collect what has passed, decide for this launch */
static RtContext::Tuner::Probe* tune_launch(RtContext* ctx, KArgs& a, bool staged, int nFrames, long long framesSinceResize)
{
    RtContext::Tuner& tn = ctx->tuner;
    RtContext::Tuner::Probe* probe = nullptr;
    a.suspendNum = tn.decided;
    if (!tn.done) {
        for (auto& pr : tn.probe)
            if (pr.live && hipEventQuery(pr.stop) == hipSuccess) {
                float ms = 0;
                if (hipEventElapsedTime(&ms, pr.start, pr.stop) == hipSuccess && pr.frames > 0) {
                    tn.ms[pr.cand] += ms / pr.frames;
                    tn.n[pr.cand]++;
                }
                pr.live = false;
            }
        if (const int decided = rt_plan::tuner_decision(tn.ms, tn.n)) {
            tn.decided = decided;
            tn.done = true;
            a.suspendNum = tn.decided;
            if (ctx->verbose) fprintf(stderr, "[raytrace_hip] launch tuner: 3/8 %.3f ms/frame, 4/8 %.3f ms/frame -> %d/8\n", tn.ms[0] / tn.n[0], tn.ms[1] / tn.n[1], tn.decided);
        } else if (rt_plan::tuner_samples(ctx->flatScene, staged, nFrames, ctx->stats, framesSinceResize)) {
            for (auto& pr : tn.probe)
                if (!pr.live) { probe = &pr; break; }
            if (probe) {
                if (!probe->start) { hipEventCreate(&probe->start); hipEventCreate(&probe->stop); }
                probe->cand = tn.next;
                probe->frames = nFrames;
                tn.next ^= 1;
                a.suspendNum = probe->cand ? 4 : 3;
            }
        }
    }
    /* frames per fused launch (RT_FUSE_MIN ...): the cap the NEXT batches are cut to */
    if (!ctx->fuseCapPinned)
        for (auto& fp : ctx->fuseProbe) {
            if (!fp.live || hipEventQuery(fp.stop) != hipSuccess) continue;
            fp.live = false;
            if (fp.frames <= 0) continue;
            float ms = 0;
            /* the previous fused launch's end to this one's; no predecessor (the first fused launch, a chain broken by full probes): its own
             * start to its end (includes what it waited for the other stream's kernels: over-estimates, i.e. errs towards shorter batches).
             * (a slot re-recorded by a later launch gives a negative or failing difference: skipped) */
            hipEvent_t from = fp.prev >= 0 ? ctx->fuseProbe[fp.prev].stop : fp.start;
            if (!from || hipEventElapsedTime(&ms, from, fp.stop) != hipSuccess || !(ms > 0)) { (void)hipGetLastError(); continue; }
            const rt_plan::FuseCap fc = rt_plan::fuse_cap(ms, fp.frames, (size_t)ctx->localRows * ctx->W, ctx->stagingBytes);
            if (fc.cap != ctx->fuseCap && ctx->verbose) fprintf(stderr, "[raytrace_hip] fused launches: %.3f ms per frame -> up to %d frames per launch\n", fc.msPerFrame, fc.cap);
            ctx->fuseCap = fc.cap;
        }
    return probe;
}
/* around the trace kernel of a fused launch: returns the probe slot (or -1) */
static int mark_fused_launch_begin(RtContext* ctx, hipStream_t st)
{
    if (ctx->fuseCapPinned) return -1;
    int slot = -1;
    for (int i = 0; i < (int)(sizeof(ctx->fuseProbe) / sizeof(ctx->fuseProbe[0])); i++)
        if (!ctx->fuseProbe[i].live && i != ctx->fuseLast) { slot = i; break; }
    if (slot < 0) { ctx->fuseLast = -1; return -1; } /* all in flight: the chain of stop events breaks here */
    RtContext::FuseProbe& fp = ctx->fuseProbe[slot];
    if (!fp.stop) { hipEventCreate(&fp.start); hipEventCreate(&fp.stop); }
    if (!fp.start || !fp.stop) return -1;
    if (ctx->fuseLast < 0 && hipEventRecord(fp.start, st) != hipSuccess) return -1; /* only a launch without a predecessor needs its own start */
    return slot;
}
static void mark_fused_launch_end(RtContext* ctx, int slot, hipStream_t st, int nFrames)
{
    if (slot < 0) return;
    RtContext::FuseProbe& fp = ctx->fuseProbe[slot];
    if (hipEventRecord(fp.stop, st) == hipSuccess) {
        fp.frames = nFrames;
        fp.prev = ctx->fuseLast; /* its event stays recorded (a slot is reused only when it is not the last one) */
        fp.live = true;
        ctx->fuseLast = slot;
    }
}

/* ---- HipOrder: the steps LaunchOrder::run issues, on HIP streams and events */
struct LaunchJob {
    KArgs& a;
    const LaunchPlan& plan;
    int tiles, nFrames;
    size_t nPix;
    RtContext::Tuner::Probe* probe;
};

hipStream_t HipOrder::stream(int s) const { return s ? ctx->sideStream : ctx->stream; }

int HipOrder::record(rt_order::Event e, int s)
{
    HIP_TRY(ctx, hipEventRecord(ev[e], stream(s)));
    return RT_OK;
}

int HipOrder::wait(int s, rt_order::Event e)
{
    HIP_TRY(ctx, hipStreamWaitEvent(stream(s), ev[e], 0));
    return RT_OK;
}

int HipOrder::sort(int s, int target)
{
    hipLaunchKernelGGL(rtk::rt_order_kernel, dim3(1), dim3(1024), 0, stream(s), ctx->dTileCost, ctx->dTileKey, ctx->dTileOrder[target], job->tiles);
    HIP_TRY(ctx, hipGetLastError());
    return RT_OK;
}

/* The trace kernel of part `part` of a launch: persistent waves over (tile, frame group) items, their count, grid and tile-queue
 * bookkeeping from rt_plan::plan_part.
 * Two parts on two streams for a single frame while the context runs on its own stream: a kernel ends with a drain phase as long as one
 * pixel's serial chain, during which waves retire one by one; the other stream's kernel — different pixels, no dependence — picks up
 * every slot that frees.  With a caller-provided stream the caller's stream order is the contract: one kernel on that stream. */
int HipOrder::trace(int s, int p, int parts)
{
    KArgs& a = job->a;
    const LaunchPlan& plan = job->plan;
    const int nFrames = job->nFrames;
    rt_plan::Work w;
    w.tiles = job->tiles;
    w.nFrames = nFrames;
    w.flat = ctx->flatScene;
    w.spp = ctx->params.numRaysPerPixel;
    w.frameGroupOverride = ctx->frameGroupOverride;
    w.gridOverride = ctx->gridOverride;
    w.residentGroups = plan.resident;
    w.wavesPerGroup = plan.shape.wavesPerGroup;
    const rt_plan::PartPlan pp = rt_plan::plan_part(w, p, parts, ctx->tileQueueNext[s]);
    a.tileOrder = ctx->order.orderValid ? ctx->dTileOrder[ctx->order.orderCur] : nullptr; /* (a sort of this launch may just have written it) */
    a.frameGroup = pp.frameGroup;
    a.frameGroupShift = pp.frameGroupShift;
    a.frameGroups = pp.frameGroups;
    a.launchTiles = pp.partTiles;
    a.launchItems = (int)pp.items;
    a.orderOffset = p;
    a.orderStride = parts;
    a.queueStart = pp.queueStart;
    if (ctx->verbose) fprintf(stderr, "[raytrace_hip] launch variant=%d part=%d/%d tiles=%d grid=%d x %d waves perCU=%d lds=%zu\n", plan.shape.variant, p, parts, pp.partTiles, pp.grid, plan.shape.wavesPerGroup, ctx->occPerCU[plan.shape.variant], plan.shape.ldsBytes);
    /* the stream's pixel-record slot and tile-queue counter */
    hipStream_t st = stream(s);
    a.pxCold = (float4*)((char*)ctx->dPxCold + (size_t)s * ctx->pxColdWaves * RT_COLD_STRIDE_BYTES);
    a.tileQueue = ctx->dTileQueue + s;
    a.tileQueueBase = pp.tileQueueBase;
    /* this stream's table of per-tile sphere candidates: refilled here, in stream order in front of its reader, when it holds another key's masks */
    a.tileCand = nullptr;
    if (ctx->tileCandWanted && ctx->tileCandTiles == job->tiles && ctx->tileCandWant.tiles == job->tiles) {
        if (!ctx->tileCandValid[s] || memcmp(&ctx->tileCandKey[s], &ctx->tileCandWant, sizeof(TileCandKey)) != 0) {
            ctx->tileCandValid[s] = false;
            hipLaunchKernelGGL(rtk::rt_tile_cand_kernel, dim3((unsigned)((job->tiles + 255) / 256)), dim3(256), 0, st, ctx->tileCandWant, ctx->dTileCand[s]);
            HIP_TRY(ctx, hipGetLastError());
            ctx->tileCandKey[s] = ctx->tileCandWant;
            ctx->tileCandValid[s] = true;
        }
        a.tileCand = ctx->dTileCand[s];
        ctx->lastTileCand = 1;
        ctx->lastTileTri = ctx->tileCandWant.triOn;
    }
    RtContext::Tuner::Probe* probe = job->probe;
    const int fuseSlot = nFrames > 1 ? mark_fused_launch_begin(ctx, st) : -1;
    if (probe) hipEventRecord(probe->start, st);
    hipLaunchKernelGGL(parts == 2 ? plan.kernHalf : plan.kern, dim3(pp.grid), dim3(plan.shape.blockThreads), plan.shape.ldsBytes, st, a);
    if (probe) { hipEventRecord(probe->stop, st); probe->live = true; }
    HIP_TRY(ctx, hipGetLastError()); /* a refused launch ran no wave: the device counter did not move */
    mark_fused_launch_end(ctx, fuseSlot, st, nFrames);
    ctx->tileQueueNext[s] = pp.queueNext;
    return RT_OK;
}

/* RCC:18-23 for a fused launch's frames, in frame order */
int HipOrder::accumulate(int s)
{
    int blocks = (int)((job->nPix + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(rtk::rt_accumulate_kernel, dim3(blocks), dim3(256), 0, stream(s), (const float4*)ctx->dStaging[s], job->nFrames, job->nPix,
                       (float4*)job->a.accumulated, (float4*)job->a.frameRender, job->nPix);
    HIP_TRY(ctx, hipGetLastError());
    return RT_OK;
}

static int launch_frames(RtContext* ctx, int frame0, int nFrames)
{
    KArgs a;
    fill_args(ctx, frame0, nFrames, a, true, true);
    const int tiles = a.tilesX * a.tilesY;
    if (tiles == 0) return RT_OK;
    LaunchPlan plan;
    int rc = choose_variant(ctx, a, plan);
    if (rc) return rc;
    if ((rc = prepare_records(ctx, plan))) return rc;
    if ((rc = prepare_tile_order(ctx, a, tiles))) return rc;
    if ((rc = prepare_tile_cand(ctx, tiles))) return rc;
    /* Fused launches (several frames: (tile, frame) items, per-frame colours staged and summed in frame order afterwards) alternate
     * between the context's two streams (own streams only), each with its own staging slab: the trace kernel of launch k+1 — other
     * frames, nothing shared but the scene — starts while launch k drains, and only the rt_accumulate_kernels, which add into the
     * accumulation buffer in FRAME order, are chained by events.
     * Two kernels sharing the chip refill each other's freed wave slots one by one — with single-wave workgroups.  A 12-wave workgroup frees
     * its slots and its LDS only when its LAST wave ends, and the other kernel's workgroups need twelve slots at once: overlapping launches then
     * wait for each other instead of filling gaps (config 4 / 5: 7.8 / 50.2 ms per frame for K back-to-back rt_render_frame against 6.2 / 42.1 on
     * one stream, profiles/r06_groups_and_streams.txt).  The BVH variants' group launches therefore stay on ONE stream, one kernel per launch. */
    rt_order::Shape shape;
    shape.frames = nFrames;
    shape.singleWave = plan.shape.wavesPerGroup == 1;
    shape.tiles = tiles;
    const rt_order::Placement pl = ctx->order.place(shape);
    const size_t nPix = (size_t)ctx->localRows * ctx->W;
    if (pl.staged) {
        bool unavailable = false;
        if ((rc = prepare_staging(ctx, a, nFrames, nPix, pl.lane, pl.split, &unavailable))) return rc;
        if (unavailable) {
            if (pl.lane == 1) { /* no room for the second slab: every fused launch on the main stream from now on */
                ctx->order.alternate = false;
                ctx->order.stagedNext = 0;
                return launch_frames(ctx, frame0, nFrames);
            }
            /* not even one slab: the frames go out one launch each (a single-frame launch needs no staging) — a render call never
             * fails for want of scratch — and the allocation is not tried again until the image is resized */
            ctx->stagingUnavailable = true;
            for (int f = 0; f < nFrames; f++)
                if ((rc = launch_frames(ctx, frame0 + f, 1))) return rc; /* each counts itself in ctx->lastLaunched */
            return RT_OK;
        }
    }
    LaunchJob job{a, plan, tiles, nFrames, nPix, tune_launch(ctx, a, pl.staged, nFrames, pl.framesAfter)};
    ctx->backend.job = &job;
    rc = ctx->order.run(pl, ctx->backend);
    ctx->backend.job = nullptr;
    if (rc) return rc;
    ctx->pixelFrames += (uint64_t)ctx->localRows * ctx->W * nFrames;
    ctx->lastLaunched += nFrames;
    return RT_OK;
}

int check_renderable(RtContext* ctx)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    if (ctx->W == 0) return fail(ctx, RT_ERR_STATE, "render before rt_resize");
    if (!ctx->haveScene) return fail(ctx, RT_ERR_STATE, "render before rt_upload_scene");
    if (!ctx->haveParams) return fail(ctx, RT_ERR_STATE, "render before rt_set_params");
    if (ctx->params.numRaysPerPixel < 0) return fail(ctx, RT_ERR_INVALID_ARG, "numRaysPerPixel < 0");
    return RT_OK;
}

static bool gpu_idle(RtContext* ctx)
{
    if (ctx->holdBack) return false;
    if (hipStreamQuery(ctx->stream) != hipSuccess) return false;
    if (ctx->sideStream && ctx->order.sideDirty && hipStreamQuery(ctx->sideStream) != hipSuccess) return false;
    return true;
}

extern "C" {

int rt_render_frame(RtContext* ctx)
{
    int rc = check_renderable(ctx);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    /* Frames requested while earlier ones still execute are held back and leave as one fused launch (each pixel
     * runs its frames back to back: same bits as one launch per frame, without a chip-wide drain per frame) when
     * fuseCap have gathered or at the next call that needs them.  An idle GPU starts at once. */
    if (ctx->coalesce && ctx->fuseFrames && ctx->params.accumulate && ctx->stream == ctx->ownStream) {
        if (gpu_idle(ctx)) {
            RT_FLUSH(ctx);
            rc = launch_frames(ctx, ctx->frame, 1);
            if (rc) return rc;
            ctx->frame++;
            return RT_OK;
        }
        ctx->pending++;
        ctx->frame++; /* RCM:94 */
        if (ctx->pending >= ctx->fuseCap) RT_FLUSH(ctx);
        return RT_OK;
    }
    RT_FLUSH(ctx);
    rc = launch_frames(ctx, ctx->frame, 1);
    if (rc) return rc;
    if (ctx->params.accumulate) ctx->frame++; /* RCM:94 */
    return RT_OK;
}

/* Launch what rt_render_frame holds back, without waiting for it. */
int rt_flush(RtContext* ctx)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    RT_FLUSH(ctx);
    return RT_OK;
}

int rt_render_frames(RtContext* ctx, int n)
{
    int rc = check_renderable(ctx);
    if (rc) return rc;
    if (n < 0) return fail(ctx, RT_ERR_INVALID_ARG, "rt_render_frames: n < 0");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RT_FLUSH(ctx);
    if (ctx->fuseFrames && ctx->params.accumulate) {
        /* Batched form: each pixel runs its frames back to back inside one launch — same Frame
         * seeds, same order of additions into the sum, FrameRender = the last frame — so the
         * chip-wide drain at the end of a launch is paid once per batch instead of once per
         * frame.  Batches are capped to keep launches short. */
        while (n > 0) {
            const int k = n < ctx->fuseCap ? n : ctx->fuseCap;
            rc = launch_frames(ctx, ctx->frame, k);
            if (rc) return rc;
            ctx->frame += k;
            n -= k;
        }
        return RT_OK;
    }
    for (int i = 0; i < n; i++) {
        rc = launch_frames(ctx, ctx->frame, 1);
        if (rc) return rc;
        if (ctx->params.accumulate) ctx->frame++;
    }
    return RT_OK;
}

int rt_synchronize(RtContext* ctx)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    RT_FLUSH(ctx);
    HIP_TRY(ctx, hipStreamSynchronize(joined(ctx)));
    flush_timer(ctx);
    for (SidePass& sp : ctx->side) /* a device-form side pass completes here: so does its watchdog report (no-op otherwise) */
        if (int rc = side_report(ctx, sp, "rt_synchronize")) return rc;
    return RT_OK;
}

int rt_get_frame(const RtContext* ctx) { return ctx ? ctx->frame : RT_ERR_INVALID_ARG; }

int rt_timer_begin(RtContext* ctx)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    RT_FLUSH(ctx);
    flush_timer(ctx);
    if (ctx->timerState == 1) return fail(ctx, RT_ERR_STATE, "rt_timer_begin: timer already running");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventRecord(ctx->evStart, joined(ctx)));
    ctx->timerState = 1;
    return RT_OK;
}
int rt_timer_end(RtContext* ctx)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    RT_FLUSH(ctx);
    if (ctx->timerState != 1) return fail(ctx, RT_ERR_STATE, "rt_timer_end without rt_timer_begin");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventRecord(ctx->evStop, joined(ctx)));
    ctx->timerState = 2;
    return RT_OK;
}

static int read_target(RtContext* ctx, int use_accumulated, float* rgba, size_t bytes)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    RT_FLUSH(ctx);
    if (int rc = check_rows_buffer(ctx, "rt_read", 16, rgba, bytes, true)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(joined(ctx)));
    flush_timer(ctx);
    if (int rc = check_watchdog(ctx, ctx, "rt_read")) return rc;
    if (bytes) HIP_TRY(ctx, hipMemcpy(rgba, image_target(ctx, use_accumulated), bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}
int rt_read_frame(RtContext* ctx, float* rgba, size_t bytes) { return read_target(ctx, 0, rgba, bytes); }
int rt_read_accumulated(RtContext* ctx, float* rgba, size_t bytes) { return read_target(ctx, 1, rgba, bytes); }

/* ---- display pass + checkpoint ------------------------------------------------ */
/* rt_display (srgb8 = false: RGBA32F) and rt_display_srgb8 (RGBA8, optionally flipped): they differ in the kernel and the pixel size */
static int display_pass(RtContext* ctx, const char* call, bool srgb8, int frame, int use_accumulated, int flip_y, void* out, size_t bytes)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    RT_FLUSH(ctx);
    if (ctx->W == 0) return fail(ctx, RT_ERR_STATE, "display before rt_resize");
    if (frame == 0) return fail(ctx, RT_ERR_INVALID_ARG, "display: Frame must not be 0");
    int rc = check_rows_buffer(ctx, call, srgb8 ? 4 : 16, out, bytes, true);
    if (rc) return rc;
    const size_t n = (size_t)ctx->localRows * ctx->W;
    if (n == 0) return RT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = grow_scratch(ctx, &ctx->dDisplay, &ctx->displayBytes, bytes))) return rc;
    int blocks = (int)((n + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    const float4* src = (const float4*)image_target(ctx, use_accumulated);
    if (srgb8) hipLaunchKernelGGL(rtk::rt_display_srgb8_kernel, dim3(blocks), dim3(256), 0, joined(ctx), src, (uint32_t*)ctx->dDisplay, ctx->W, ctx->localRows, frame, flip_y);
    else hipLaunchKernelGGL(rtk::rt_display_kernel, dim3(blocks), dim3(256), 0, joined(ctx), src, (float4*)ctx->dDisplay, n, frame);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(joined(ctx));
    if (e == hipSuccess && (rc = check_watchdog(ctx, ctx, call))) return rc;
    if (e == hipSuccess) e = hipMemcpy(out, ctx->dDisplay, bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(ctx, RT_ERR_HIP, "%s: %s", call, hipGetErrorString(e));
    return RT_OK;
}

int rt_display(RtContext* ctx, int frame, int use_accumulated, float* rgba, size_t bytes)
{
    return display_pass(ctx, "rt_display", false, frame, use_accumulated, 0, rgba, bytes);
}

int rt_display_srgb8(RtContext* ctx, int frame, int use_accumulated, int flip_y, uint8_t* rgba8, size_t bytes)
{
    return display_pass(ctx, "rt_display_srgb8", true, frame, use_accumulated, flip_y, rgba8, bytes);
}

int rt_write_accumulated(RtContext* ctx, const float* rgba, size_t bytes)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    RT_FLUSH(ctx);
    if (int rc = check_rows_buffer(ctx, "rt_write_accumulated", 16, rgba, bytes, true)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(joined(ctx)));
    if (bytes) HIP_TRY(ctx, hipMemcpy(accum_target(ctx), rgba, bytes, hipMemcpyHostToDevice));
    return clear_watchdog(ctx); /* the accumulated image is the caller's checkpoint now */
}

int rt_enable_stats(RtContext* ctx, int enabled)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    RT_FLUSH(ctx);
    ctx->stats = enabled != 0;
    return RT_OK;
}

int rt_reset_counters(RtContext* ctx)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    RT_FLUSH(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(joined(ctx)));
    flush_timer(ctx);
    /* stream-ordered: the next launch on this stream starts after the fill (a null-stream hipMemset is not ordered
     * against the non-blocking render streams and may land after the next kernel's first waves have counted).
     * Every word but the watchdog word: the images it condemns are still in the targets (clear_watchdog) */
    const size_t words = (size_t)RT_COUNTER_SLOTS * RT_COUNTER_FIELDS;
    HIP_TRY(ctx, hipMemsetAsync(ctx->dCounters, 0, sizeof(unsigned long long) * kWatchdogWord, joined(ctx)));
    HIP_TRY(ctx, hipMemsetAsync(ctx->dCounters + kWatchdogWord + 1, 0, sizeof(unsigned long long) * (words - kWatchdogWord - 1), joined(ctx)));
    ctx->pixelFrames = 0;
    ctx->gpuMs = 0;
    return RT_OK;
}

/* After a synchronise of the joined stream: the whole counter block on the host; sum_field adds one field up over the slots */
static int read_counter_block(RtContext* ctx, std::vector<unsigned long long>& h)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(joined(ctx)));
    h.resize((size_t)RT_COUNTER_SLOTS * RT_COUNTER_FIELDS);
    HIP_TRY(ctx, hipMemcpy(h.data(), ctx->dCounters, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return RT_OK;
}
static unsigned long long sum_field(const std::vector<unsigned long long>& h, int f)
{
    unsigned long long sum = 0;
    for (int s = 0; s < RT_COUNTER_SLOTS; s++) sum += h[(size_t)s * RT_COUNTER_FIELDS + f];
    return sum;
}

int rt_get_counters(RtContext* ctx, RtCounters* out)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    RT_FLUSH(ctx);
    if (!out) return fail(ctx, RT_ERR_INVALID_ARG, "rt_get_counters: null out");
    std::vector<unsigned long long> h;
    if (int rc = read_counter_block(ctx, h)) return rc;
    flush_timer(ctx);
    out->segments = sum_field(h, 0);
    out->innerSteps = sum_field(h, 1);
    out->leafSteps = sum_field(h, 2);
    out->triTests = sum_field(h, 3);
    out->sphereTests = sum_field(h, 4);
    out->modelVisits = sum_field(h, 5);
    out->pixelFrames = ctx->pixelFrames;
    out->gpuMs = ctx->gpuMs;
    /* word 7 = the watchdogs (rt_kernels.h): traverse — a wave ended its lanes' walks because no validated scene needs that many steps; pool_exchange — a wave
     * gave up waiting for a cell of the FLAT variant's chain pool.  Not cleared by rt_reset_counters (clear_watchdog) */
    if (h[kWatchdogWord]) return fail(ctx, RT_ERR_HIP, "a kernel watchdog fired %llu times: a traversal did not end (scene validation has a hole, or device memory is corrupt) or, in a scene without trees, a cell of the chain pool was never handed over; the images since the last rt_reset_accumulation / rt_write_accumulated / rt_resize are not valid", h[kWatchdogWord]);
    return RT_OK;
}

/* ---- test hooks ------------------------------------------------------------ */
/* Wave-level phase profile of the stats launches since rt_reset_counters:
 * out[2*p] = times a wave executed phase p, out[2*p+1] = lanes active in it
 * (p: 0 loop, 1 raygen, 2 spheres, 3 traverse call, 4 model setup, 5 inner step,
 *  6 triangle test, 7 shade hit, 8 sky, 9 sphere roots, 10 glass branch, 11 pixel refill). */
int rt_debug_phase_profile(RtContext* ctx, uint64_t* out, int n)
{
    if (!ctx || !out || n < 2 * RT_N_PHASES) return fail(ctx, RT_ERR_INVALID_ARG, "rt_debug_phase_profile: need %d entries", 2 * RT_N_PHASES);
    RT_FLUSH(ctx);
    std::vector<unsigned long long> h;
    if (int rc = read_counter_block(ctx, h)) return rc;
    for (int f = 0; f < 2 * RT_N_PHASES; f++) out[f] = sum_field(h, 8 + f);
    if (n > 2 * RT_N_PHASES) out[2 * RT_N_PHASES] = sum_field(h, 6); /* audit of the conservative root filter: must be 0 */
    /* then: inner steps served by the LDS top-of-tree cache; inner steps (lane-steps) taken while >= 48 lanes of the wave stood on ONE node;
     * the same for >= 3/4 of >= 16 active lanes; the rest 0 */
    for (int p = 0; p < RT_N_PHASES && 2 * RT_N_PHASES + 1 + p < n; p++) out[2 * RT_N_PHASES + 1 + p] = p < 3 ? sum_field(h, 8 + 2 * RT_N_PHASES + p) : 0;
    return RT_OK;
}

/* device scratch that is released on every exit path of the two hooks below */
struct DevScratch {
    void* p = nullptr;
    ~DevScratch() { if (p) hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
    float* f() const { return (float*)p; }
};

int rt_debug_fused_frames_cap(const RtContext* ctx) { return ctx ? ctx->fuseCap : RT_ERR_INVALID_ARG; }
int rt_debug_pending_frames(const RtContext* ctx) { return ctx ? ctx->pending : RT_ERR_INVALID_ARG; }
int rt_debug_primary_table(const RtContext* ctx) { return ctx ? ctx->lastPrimaryOn : RT_ERR_INVALID_ARG; }
int rt_debug_tile_cand(const RtContext* ctx) { return ctx ? ctx->lastTileCand : RT_ERR_INVALID_ARG; }
int rt_debug_tile_tri(const RtContext* ctx) { return ctx ? ctx->lastTileTri : RT_ERR_INVALID_ARG; }

int rt_debug_intersect(RtContext* ctx, const float* origins, const float* dirs, int n, float* out10)
{
    if (ctx) RT_FLUSH(ctx);
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    if (!ctx->haveScene) return fail(ctx, RT_ERR_STATE, "rt_debug_intersect before rt_upload_scene");
    if (n < 0 || (n && (!origins || !dirs || !out10))) return fail(ctx, RT_ERR_INVALID_ARG, "rt_debug_intersect: bad arguments");
    if (n == 0) return RT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevScratch dO, dD, dR;
    HIP_TRY(ctx, dO.alloc((size_t)n * 12));
    HIP_TRY(ctx, dD.alloc((size_t)n * 12));
    HIP_TRY(ctx, dR.alloc((size_t)n * 40));
    HIP_TRY(ctx, hipMemcpy(dO.p, origins, (size_t)n * 12, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(dD.p, dirs, (size_t)n * 12, hipMemcpyHostToDevice));
    KArgs a;
    fill_args(ctx, 1, 1, a);
    hipLaunchKernelGGL(rtk::rt_debug_intersect_kernel, dim3((n + RT_WAVE - 1) / RT_WAVE), dim3(RT_WAVE), 0, joined(ctx), a, dO.f(), dD.f(), n, dR.f());
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(joined(ctx)));
    HIP_TRY(ctx, hipMemcpy(out10, dR.p, (size_t)n * 40, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_debug_math_eval(RtContext* ctx, int op, const float* x, const float* y, float* out, int n)
{
    if (ctx) RT_FLUSH(ctx);
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    if (n < 0 || (n && (!x || !y || !out))) return fail(ctx, RT_ERR_INVALID_ARG, "rt_debug_math_eval: bad arguments");
    if (n == 0) return RT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevScratch dX, dY, dR;
    HIP_TRY(ctx, dX.alloc((size_t)n * 4));
    HIP_TRY(ctx, dY.alloc((size_t)n * 4));
    HIP_TRY(ctx, dR.alloc((size_t)n * 4));
    HIP_TRY(ctx, hipMemcpy(dX.p, x, (size_t)n * 4, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(dY.p, y, (size_t)n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(rtk::rt_debug_math_kernel, dim3((n + 255) / 256), dim3(256), 0, joined(ctx), op, dX.f(), dY.f(), dR.f(), n);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(joined(ctx)));
    HIP_TRY(ctx, hipMemcpy(out, dR.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return RT_OK;
}

/* ---- the passes that trace as single waves (rt_render_cost, the side passes): no top-of-tree cache, no chain pool ----------------
 * The KArgs fields of that form, the LDS attribute a wave region above 48 KB needs, and *residentWaves = every wave the device keeps
 * resident.  waveLdsBytes is the caller's: the cost kernel's FLAT form keeps its pixel records in LDS (rt_plan::launch_shape adds them),
 * the side passes' kernels have none (rt_plan::wave_lds_bytes). */
static int single_wave_pass(RtContext* ctx, const void* kern, size_t waveLdsBytes, KArgs& a, long long* residentWaves)
{
    a.wavesPerGroup = 1;
    a.hotUnits = 0;
    a.poolCells = 0;
    a.waveLdsDwords = (int)(waveLdsBytes / sizeof(uint32_t));
    a.stackEntries = ctx->stackEntries;
    if (waveLdsBytes > 48 * 1024) HIP_TRY(ctx, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)waveLdsBytes));
    int perCU = 0;
    HIP_TRY(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kern, RT_WAVE, waveLdsBytes));
    *residentWaves = (long long)(perCU > 0 ? perCU : 1) * ctx->numCUs;
    return RT_OK;
}

/* The instantiation of a single-wave kernel K<FLAT, MANY, ...> for the context's scene: MANY (more than 64 models), FLAT (every root a
 * leaf) or the plain BVH form; further template arguments follow K */
#define RT_SCENE_KERNEL(ctx, K, ...)                                                                      \
    (rt_plan::many_models((ctx)->nChunks, (ctx)->flatScene) ? K<false, true, ##__VA_ARGS__>               \
     : (ctx)->flatScene                                     ? K<true, false, ##__VA_ARGS__>               \
                                                            : K<false, false, ##__VA_ARGS__>)

/* ---- rt_render_cost (include/rt_cost.h): per-pixel work of one frame ----------------------
 * The stats build of the trace kernel in its single-wave, unpooled form without the top-of-tree cache (rt_kernels.h, rt_cost_kernel):
 * one lane owns a pixel from set-up to finish, so the lane's exact counters between the two are that pixel's.  The launch is the
 * context's in nothing but the scene, the parameters and the stream: its own tile counter, identity tile order, no tile costs, no
 * pixel-record slot of the render streams, and a counter block of its own — RtCounters and the watchdog word of the context stay as they
 * are, and a watchdog that fires here fails this call only. */
int rt_render_cost(RtContext* ctx, int frame, RtPixelCost* out, size_t bytes)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    if (frame < 1) return fail(ctx, RT_ERR_INVALID_ARG, "rt_render_cost: frame %d < 1 (the first frame after a reset is 1)", frame);
    int rc = check_renderable(ctx);
    if (rc) return rc;
    if ((rc = check_rows_buffer(ctx, "rt_render_cost", sizeof(RtPixelCost), out, bytes))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RT_FLUSH(ctx);
    KArgs a;
    fill_args(ctx, frame, 1, a, false, true);
    const int tiles = a.tilesX * a.tilesY;
    if (tiles == 0) return RT_OK;
    rt_plan::SceneShape sc; /* no cache, no pool: single waves */
    sc.flat = ctx->flatScene;
    sc.stats = true;
    sc.stackEntries = ctx->stackEntries;
    sc.extWords = ctx->extWords;
    sc.nChunks = ctx->nChunks;
    sc.numCUs = ctx->numCUs;
    const rt_plan::LaunchShape sh = rt_plan::launch_shape(sc, tiles, 1);
    void (*kern)(const KArgs, uint32_t*) = RT_SCENE_KERNEL(ctx, rtk::rt_cost_kernel); /* (sh.many is the same rt_plan::many_models) */
    a.suspendNum = ctx->tuner.decided; /* scheduling only: the counts of a ray do not depend on it */
    long long resident = 0;
    if ((rc = single_wave_pass(ctx, reinterpret_cast<const void*>(kern), sh.ldsBytes, a, &resident))) return rc; /* (one wave per group: the group's LDS is the wave's) */
    rt_plan::Work w;
    w.tiles = tiles;
    w.nFrames = 1;
    w.flat = ctx->flatScene;
    w.spp = ctx->params.numRaysPerPixel;
    w.residentGroups = resident;
    w.wavesPerGroup = 1;
    const rt_plan::PartPlan pp = rt_plan::plan_part(w, 0, 1, 0ull); /* one kernel, a tile counter that starts at 0 */
    a.tileOrder = nullptr;
    a.tileCost = nullptr;
    a.frameGroup = pp.frameGroup;
    a.frameGroupShift = pp.frameGroupShift;
    a.frameGroups = pp.frameGroups;
    a.launchTiles = pp.partTiles;
    a.launchItems = (int)pp.items;
    a.orderOffset = 0;
    a.orderStride = 1;
    a.queueStart = pp.queueStart;
    a.tileQueueBase = pp.tileQueueBase;
    /* [0, RT_COUNTER_FIELDS): the launch's counter slot (only the watchdog word is written), then the tile counter */
    DevScratch dWords, dCold, dOut;
    HIP_TRY(ctx, dWords.alloc(sizeof(unsigned long long) * (RT_COUNTER_FIELDS + 1)));
    if (!ctx->flatScene) HIP_TRY(ctx, dCold.alloc((size_t)pp.grid * RT_COLD_STRIDE_BYTES)); /* (the FLAT variant keeps its pixel records in LDS) */
    HIP_TRY(ctx, dOut.alloc(bytes));
    unsigned long long* const words = (unsigned long long*)dWords.p;
    a.counters = words;
    a.tileQueue = words + RT_COUNTER_FIELDS;
    a.pxCold = (float4*)dCold.p;
    hipStream_t st = joined(ctx);
    HIP_TRY(ctx, hipMemsetAsync(words, 0, sizeof(unsigned long long) * (RT_COUNTER_FIELDS + 1), st));
    HIP_TRY(ctx, hipMemsetAsync(dOut.p, 0, bytes, st));
    hipLaunchKernelGGL(kern, dim3(pp.grid), dim3(RT_WAVE), sh.ldsBytes, st, a, (uint32_t*)dOut.p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));
    unsigned long long fired = 0;
    HIP_TRY(ctx, hipMemcpy(&fired, words + kWatchdogWord, sizeof(fired), hipMemcpyDeviceToHost));
    if (fired) return watchdog_failure(ctx, "rt_render_cost", fired);
    HIP_TRY(ctx, hipMemcpy(out, dOut.p, bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

} /* extern "C" */

/* ---- rt_adaptive_render_frames (include/rt_adaptive.h; the entry points are rt_post.hip's): the frames of a tile list ------------
 * The kernels of the selection and of the list's accumulate step are rt_adaptive.hip's (rt_ad::enqueue_*); the frames themselves are the
 * production trace kernel choose_variant picks, launched over the list: ONE kernel on the joined main stream, whose queue position q is
 * entry q of the list (tileOrder = the list, orderOffset / orderStride = 0 / 1), launchItems from rt_plan::plan_part with tiles = the
 * list's length, tileCost = null (the cost records that order the normal launches are not skewed by partial frames), the main stream's
 * pixel-record slot and staging slab (stream order), and a tile counter of its own.  ctx->order sees a join and nothing else; the
 * tuner and the fuse probes are not touched. */
/* Frames frame0 ... frame0 + nFrames - 1 of the current (non-empty) list: one trace kernel and, for nFrames > 1, the list's accumulate
 * step.  *unstaged = true (and nothing enqueued) when nFrames > 1 and there is no staging slab for them. */
int adaptive_launch(RtContext* ctx, int frame0, int nFrames, bool* unstaged)
{
    *unstaged = false;
    KArgs a;
    fill_args(ctx, frame0, nFrames, a, true, true);
    LaunchPlan plan;
    int rc = choose_variant(ctx, a, plan);
    if (rc) return rc;
    if ((rc = prepare_records(ctx, plan))) return rc;
    const size_t nPix = (size_t)ctx->localRows * ctx->W;
    if (nFrames > 1) {
        if ((rc = prepare_staging(ctx, a, nFrames, nPix, 0, false, unstaged))) return rc;
        if (*unstaged) return RT_OK;
    }
    if (!ctx->dAdQueue) {
        HIP_TRY(ctx, hipMalloc(&ctx->dAdQueue, sizeof(unsigned long long)));
        HIP_TRY(ctx, hipMemsetAsync(ctx->dAdQueue, 0, sizeof(unsigned long long), joined(ctx)));
        ctx->adQueueNext = 0;
    }
    a.suspendNum = ctx->tuner.decided; /* scheduling only; the tuner itself is not sampled by these launches */
    rt_plan::Work w;
    w.tiles = (int)ctx->adTilesActive;
    w.nFrames = nFrames;
    w.flat = ctx->flatScene;
    w.spp = ctx->params.numRaysPerPixel;
    w.frameGroupOverride = ctx->frameGroupOverride;
    w.gridOverride = ctx->gridOverride;
    w.residentGroups = plan.resident;
    w.wavesPerGroup = plan.shape.wavesPerGroup;
    const rt_plan::PartPlan pp = rt_plan::plan_part(w, 0, 1, ctx->adQueueNext);
    a.tileOrder = ctx->dAdTiles;
    a.tileCost = nullptr;
    a.frameGroup = pp.frameGroup;
    a.frameGroupShift = pp.frameGroupShift;
    a.frameGroups = pp.frameGroups;
    a.launchTiles = pp.partTiles;
    a.launchItems = (int)pp.items;
    a.orderOffset = 0;
    a.orderStride = 1;
    a.queueStart = pp.queueStart;
    a.pxCold = (float4*)ctx->dPxCold; /* the main stream's slot */
    a.tileQueue = ctx->dAdQueue;
    a.tileQueueBase = pp.tileQueueBase;
    if (ctx->verbose) fprintf(stderr, "[raytrace_hip] adaptive launch variant=%d tiles=%d of %d frames=%d grid=%d x %d waves\n", plan.shape.variant, pp.partTiles, a.tilesX * a.tilesY, nFrames, pp.grid, plan.shape.wavesPerGroup);
    hipStream_t st = joined(ctx);
    hipLaunchKernelGGL(plan.kern, dim3(pp.grid), dim3(plan.shape.blockThreads), plan.shape.ldsBytes, st, a);
    HIP_TRY(ctx, hipGetLastError()); /* a refused launch ran no wave: the device counter did not move */
    ctx->adQueueNext = pp.queueNext;
    if (nFrames > 1)
        HIP_TRY(ctx, rt_ad::enqueue_accumulate_tiles(st, ctx->dAdTiles, (int)ctx->adTilesActive, ctx->W, ctx->localRows, ctx->dStaging[0], nFrames, nPix, a.accumulated,
                                                     a.frameRender));
    ctx->pixelFrames += (uint64_t)ctx->adPixelsActive * nFrames;
    return RT_OK;
}

/* ---- the side passes: the AOV pass, the ray queries and the two radiance passes -------------------------------------------------------------
 * Each is ONE launch of a single-wave kernel (rt_kernels.h) on the joined main stream — behind every frame already requested, like every
 * use of the stream that is not a render launch.  A pass is the context's in nothing but the scene, the stream and, where it reads them,
 * the parameters: KArgs from fill_args, the FLAT / MANY / BVH instantiation of its kernel (RT_SCENE_KERNEL), a wave region of the trace
 * kernel as its LDS, and no render target, tile order, tile costs, pixel records or staging slab.  Its counter slot is its own
 * (SidePass; traverse() only ever writes the slot's watchdog word), so RtCounters and the context's watchdog word stay as they
 * are, and a watchdog that fires in a pass fails that pass only.  The protocol, once:
 *     side_begin    the KArgs fields of that form, the slot (made on first use), LDS bytes and resident waves
 *     side_submit   the slot cleared, the launch and its error, in stream order
 *     side_fired / side_report / side_settle (above, with check_watchdog)   a host form reads the word when it returns; a device form
 *                   sets `unreported` and the word is handed over as described there
 * What each pass adds is stated at its enqueue function. */
static int side_begin(RtContext* ctx, SidePass& sp, const void* kern, KArgs& a, size_t* ldsBytes, long long* residentWaves)
{
    a.frameRender = nullptr;
    a.accumulated = nullptr;
    a.tileQueue = nullptr;
    a.tileOrder = nullptr;
    a.tileCost = nullptr;
    a.pxCold = nullptr;
    a.staging = nullptr;
    if (!sp.words) HIP_TRY(ctx, hipMalloc(&sp.words, sizeof(unsigned long long) * RT_COUNTER_FIELDS));
    a.counters = sp.words;
    *ldsBytes = rt_plan::wave_lds_bytes(ctx->stackEntries, ctx->extWords); /* a wave region of the trace kernel, single waves, no cache, no pool */
    return single_wave_pass(ctx, kern, *ldsBytes, a, residentWaves);
}

/* `grid` single-wave workgroups of `kern`(a, args...) */
template <class Kern, class... Args>
static int side_submit(RtContext* ctx, SidePass& sp, Kern kern, long long grid, size_t ldsBytes, const KArgs& a, Args... args)
{
    hipStream_t st = joined(ctx);
    HIP_TRY(ctx, hipMemsetAsync(sp.words, 0, sizeof(unsigned long long) * RT_COUNTER_FIELDS, st));
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(RT_WAVE), ldsBytes, st, a, args...);
    HIP_TRY(ctx, hipGetLastError());
    return RT_OK;
}

/* What the radiance pass and the NEE pass share (their enqueue functions are below): fill_args with the parameters present, the
 * pass's suspension threshold, word 0 of the pass's slot as the counter that hands out the blocks of 64 rays to the resident waves
 * (word 7 is the watchdog's), rt_radiance_launch.h's block and grid arithmetic, and `kern`(a, args...) over that grid. */
template <class Kern, class... Args>
static int path_enqueue(RtContext* ctx, int pass, int suspendNum, int n, Kern kern, Args... args)
{
    KArgs a;
    fill_args(ctx, 1, 1, a);
    a.suspendNum = suspendNum;
    SidePass& sp = ctx->side[pass];
    size_t ldsBytes = 0;
    long long resident = 0; /* every wave the device keeps resident; the blocks are handed out to them */
    if (int rc = side_begin(ctx, sp, reinterpret_cast<const void*>(kern), a, &ldsBytes, &resident)) return rc;
    a.tileQueue = sp.words; /* word 0: a launch of this pass counts no segments there */
    a.tileQueueBase = 0;
    const long long grid = rt_rd::grid(rt_rd::blocks(n), resident, ctx->gridOverride);
    return side_submit(ctx, sp, kern, grid, ldsBytes, a, args...);
}

/* ---- rt_render_aov / rt_render_aov_to_device (include/rt_aov.h): what camera ray 0 of a frame finds, per pixel -------------
 * The side pass of rt_aov_kernel: KArgs as for frame `frame`, the tiles strided over the resident waves.  frame == RT_AOV_CENTRE (0)
 * selects the pixel-centre ray of include/rt_motion.h, which reads nothing of a frame: the KArgs are then those of frame 1. */
int aov_enqueue(RtContext* ctx, int frame, void* dOut)
{
    const bool centre = frame == RT_AOV_CENTRE;
    KArgs a;
    fill_args(ctx, centre ? 1 : frame, 1, a);
    const int tiles = a.tilesX * a.tilesY;
    if (tiles == 0) return RT_OK;
    void (*kern)(const KArgs, float4*, const uint32_t*) = centre ? RT_SCENE_KERNEL(ctx, rtk::rt_aov_kernel, true) : RT_SCENE_KERNEL(ctx, rtk::rt_aov_kernel, false);
    a.suspendNum = RT_SUSPEND_NUM; /* (unused: the traversal of a pass runs to completion) */
    SidePass& sp = ctx->side[SIDE_AOV];
    size_t ldsBytes = 0;
    long long grid = 0; /* every wave the device keeps resident; the tiles are strided over them */
    if (int rc = side_begin(ctx, sp, reinterpret_cast<const void*>(kern), a, &ldsBytes, &grid)) return rc;
    if (grid > tiles) grid = tiles;
    return side_submit(ctx, sp, kern, grid, ldsBytes, a, (float4*)dOut, (const uint32_t*)ctx->dUnitTri);
}

extern "C" {

/* the frame number of the public frame calls (the centre calls pass RT_AOV_CENTRE to the shared bodies instead) */
static int aov_check_frame(RtContext* ctx, const char* call, int frame)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    if (frame < 1) return fail(ctx, RT_ERR_INVALID_ARG, "%s: frame %d < 1 (the first frame after a reset is 1)", call, frame);
    return RT_OK;
}

static int aov_check_args(RtContext* ctx, const char* call, const void* out, size_t bytes)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    int rc = check_renderable(ctx);
    if (rc) return rc;
    return check_rows_buffer(ctx, call, sizeof(RtPixelAov), out, bytes);
}

/* the host and the device variant; `frame`: >= 1 (checked by the caller), or RT_AOV_CENTRE from the centre calls */
static int aov_to_host(RtContext* ctx, const char* call, int frame, RtPixelAov* out, size_t bytes)
{
    int rc = aov_check_args(ctx, call, out, bytes);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RT_FLUSH(ctx);
    SidePass& sp = ctx->side[SIDE_AOV];
    if ((rc = side_settle(ctx, sp, call))) return rc;
    if (!bytes) return RT_OK;
    if ((rc = grow_scratch(ctx, &ctx->dAovOut, &ctx->aovOutBytes, bytes))) return rc;
    if ((rc = aov_enqueue(ctx, frame, ctx->dAovOut))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(joined(ctx)));
    unsigned long long fired = 0;
    if ((rc = side_fired(ctx, sp, &fired))) return rc;
    if (fired) return watchdog_failure(ctx, call, fired);
    HIP_TRY(ctx, hipMemcpy(out, ctx->dAovOut, bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

static int aov_to_device(RtContext* ctx, const char* call, int frame, void* d_out, size_t bytes)
{
    int rc = aov_check_args(ctx, call, d_out, bytes);
    if (rc) return rc;
    if ((uintptr_t)d_out & 15) return fail(ctx, RT_ERR_INVALID_ARG, "%s: the records must be 16-byte aligned", call);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (bytes && (rc = check_device_range(ctx, call, "d_out", d_out, bytes))) return rc; /* the kernel writes through this pointer */
    RT_FLUSH(ctx);
    SidePass& sp = ctx->side[SIDE_AOV];
    if ((rc = side_settle(ctx, sp, call))) return rc;
    if (!bytes) return RT_OK;
    if ((rc = aov_enqueue(ctx, frame, d_out))) return rc;
    sp.unreported = true;
    return RT_OK;
}

int rt_render_aov(RtContext* ctx, int frame, RtPixelAov* out, size_t bytes)
{
    if (int rc = aov_check_frame(ctx, "rt_render_aov", frame)) return rc;
    return aov_to_host(ctx, "rt_render_aov", frame, out, bytes);
}

int rt_render_aov_to_device(RtContext* ctx, int frame, void* d_out, size_t bytes)
{
    if (int rc = aov_check_frame(ctx, "rt_render_aov_to_device", frame)) return rc;
    return aov_to_device(ctx, "rt_render_aov_to_device", frame, d_out, bytes);
}

/* include/rt_motion.h, A */
int rt_render_aov_centre(RtContext* ctx, RtPixelAov* out, size_t bytes) { return aov_to_host(ctx, "rt_render_aov_centre", RT_AOV_CENTRE, out, bytes); }
int rt_render_aov_centre_to_device(RtContext* ctx, void* d_out, size_t bytes) { return aov_to_device(ctx, "rt_render_aov_centre_to_device", RT_AOV_CENTRE, d_out, bytes); }

/* ---- rt_query_closest / rt_query_occluded and their *_buffers forms (include/rt_query.h): caller-made rays against the scene ----------
 * The side pass of rt_query_kernel.  It needs neither an image nor parameters — fill_args as rt_debug_intersect calls it; the kernel
 * reads the scene fields, stackEntries and travLimit alone.  The blocks of 64 rays are strided over the resident waves; the block and
 * grid arithmetic is rt_query_launch.h's. */
static int query_enqueue(RtContext* ctx, const void* dRays, int n, void* dOut, bool any)
{
    KArgs a;
    fill_args(ctx, 1, 1, a);
    void (*kern)(const KArgs, const float4*, int, void*, const uint32_t*) = any ? RT_SCENE_KERNEL(ctx, rtk::rt_query_kernel, true) : RT_SCENE_KERNEL(ctx, rtk::rt_query_kernel, false);
    a.suspendNum = RT_SUSPEND_NUM; /* (unused: the traversal of a pass runs to completion) */
    SidePass& sp = ctx->side[SIDE_QUERY];
    size_t ldsBytes = 0;
    long long resident = 0; /* every wave the device keeps resident; the blocks are strided over them */
    if (int rc = side_begin(ctx, sp, reinterpret_cast<const void*>(kern), a, &ldsBytes, &resident)) return rc;
    const long long grid = rt_qr::grid(rt_qr::blocks(n), resident, ctx->gridOverride);
    return side_submit(ctx, sp, kern, grid, ldsBytes, a, (const float4*)dRays, n, dOut, (const uint32_t*)ctx->dUnitTri);
}
static int closest_enqueue(RtContext* ctx, const void* dRays, int n, void* dOut) { return query_enqueue(ctx, dRays, n, dOut, false); }
static int occluded_enqueue(RtContext* ctx, const void* dRays, int n, void* dOut) { return query_enqueue(ctx, dRays, n, dOut, true); }

/* ---- rt_radiance_trace / rt_radiance_trace_buffers (include/rt_radiance.h): Trace for caller-made rays -------------------------------
 * The side pass of rt_radiance_kernel: path_enqueue (the kernel reads maxBounce, useSky and the sun's fields besides the scene) with
 * the tuner's suspension threshold. */
static int radiance_enqueue(RtContext* ctx, const void* dRays, int n, void* dOut)
{
    void (*kern)(const KArgs, const float4*, int, float4*) = RT_SCENE_KERNEL(ctx, rtk::rt_radiance_kernel);
    return path_enqueue(ctx, SIDE_RADIANCE, ctx->tuner.decided /* scheduling only: a path's bits do not depend on it */, n, kern, (const float4*)dRays, n, (float4*)dOut);
}

/* ---- rt_nee_trace / rt_nee_trace_buffers / rt_nee_light_count (include/rt_nee.h) -----------------------------------
 * The light table first: rebuilt from the host mirrors when an upload or an update made it stale (rt_light_table.h), its device copy
 * uploaded through the staging ring on the joined main stream — behind every pass that still reads the old one, in front of the pass
 * that wants the new one.  A table past the cap stays dirty, so every call reports it. */
static int nee_refresh_table(RtContext* ctx, const char* call)
{
    if (!ctx->lightDirty) return RT_OK;
    rt_lt::LightTable t;
    const char* why = "";
    int rc;
    try {
        rc = rt_lt::build(ctx->hModels.data(), ctx->nModels, ctx->hCorners.data(), 9, ctx->nTris, ctx->hSpheres.data(), ctx->nSpheres, t, &why);
    } catch (const std::bad_alloc&) {
        return fail(ctx, RT_ERR_OOM, "%s: out of host memory building the light table", call);
    }
    if (rc) return fail(ctx, rc, "%s: the light table: %s", call, why);
    rt_nee::TableBytes tb;
    if ((rc = rt_nee::table_bytes((long long)t.entries.size(), (long long)t.inTable.size(), &tb, &why))) return fail(ctx, rc, "%s: the light table: %s", call, why);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = grow_scratch(ctx, &ctx->dLightTable, &ctx->lightTableBytes, tb.total))) return rc;
    char* const d = (char*)ctx->dLightTable;
    /* in pieces (rt_nee::UPLOAD_CHUNK_BYTES): a slot of the pinned ring keeps the largest upload it has seen, and a table can be 335 MB */
    auto upload = [&](size_t offset, const void* src, size_t bytes) {
        for (size_t done = 0; done < bytes; done += rt_nee::UPLOAD_CHUNK_BYTES) {
            const size_t piece = bytes - done < rt_nee::UPLOAD_CHUNK_BYTES ? bytes - done : (size_t)rt_nee::UPLOAD_CHUNK_BYTES;
            if (int urc = stage_upload(ctx, d + offset + done, (const char*)src + done, piece)) return urc;
        }
        return (int)RT_OK;
    };
    if ((rc = upload(tb.entries, t.entries.data(), t.entries.size() * sizeof(RtLightEntry)))) return rc;
    if ((rc = upload(tb.cdf, t.cdf.data(), t.cdf.size() * sizeof(float)))) return rc;
    if ((rc = upload(tb.flags, t.inTable.data(), t.inTable.size() * sizeof(uint32_t)))) return rc;
    {   /* the reverse map of this table (include/rt_mis.h), behind it on the same stream */
        std::vector<uint32_t> words;
        rt_mis::MapBytes mb;
        try {
            rt_lt::LightMap map;
            rt_lt::build_map(t, ctx->hModels.data(), ctx->nModels, ctx->nTris, ctx->nSpheres, map);
            mb = rt_mis::map_bytes(map.objects.size(), map.triangles.size());
            rt_mis::pack_map(map, words);
        } catch (const std::bad_alloc&) {
            return fail(ctx, RT_ERR_OOM, "%s: out of host memory building the light map", call);
        }
        if ((rc = grow_scratch(ctx, &ctx->dLightMap, &ctx->lightMapBytes, mb.total))) return rc;
        const size_t bytes = words.size() * sizeof(uint32_t);
        for (size_t done = 0; done < bytes; done += rt_nee::UPLOAD_CHUNK_BYTES) {
            const size_t piece = bytes - done < rt_nee::UPLOAD_CHUNK_BYTES ? bytes - done : (size_t)rt_nee::UPLOAD_CHUNK_BYTES;
            if ((rc = stage_upload(ctx, (char*)ctx->dLightMap + done, (const char*)words.data() + done, piece))) return rc;
        }
    }
    ctx->lightLayout = tb;
    ctx->lightSpheres = t.nSphere;
    ctx->lightTriangles = t.nTriangle;
    ctx->lightDirty = false;
    return RT_OK;
}

/* The side pass of rt_radiance_nee_kernel: radiance_enqueue with the table and the unit -> triangle map of the layout behind it. */
static int nee_enqueue(RtContext* ctx, const char* call, const void* dRays, int n, void* dOut)
{
    if (int rc = nee_refresh_table(ctx, call)) return rc;
    void (*kern)(const KArgs, const float4*, int, float4*, const rtk::NeeTable, const uint32_t*) = RT_SCENE_KERNEL(ctx, rtk::rt_radiance_nee_kernel);
    const char* const d = (const char*)ctx->dLightTable;
    rtk::NeeTable lt;
    lt.entries = (const float4*)(d + ctx->lightLayout.entries);
    lt.cdf = (const float*)(d + ctx->lightLayout.cdf);
    lt.inTable = (const uint32_t*)(d + ctx->lightLayout.flags);
    lt.n = ctx->lightSpheres + ctx->lightTriangles;
    return path_enqueue(ctx, SIDE_NEE, RT_SUSPEND_NUM /* (unused: both walks of the pass run to completion) */, n, kern, (const float4*)dRays, n, (float4*)dOut, lt,
                        (const uint32_t*)ctx->dUnitTri);
}

static int nee_enqueue_host(RtContext* ctx, const void* dRays, int n, void* dOut) { return nee_enqueue(ctx, "rt_nee_trace", dRays, n, dOut); }
static int nee_enqueue_buffers(RtContext* ctx, const void* dRays, int n, void* dOut) { return nee_enqueue(ctx, "rt_nee_trace_buffers", dRays, n, dOut); }

/* The side pass of rt_mis_trace (include/rt_mis.h): the MIS instantiation of rt_radiance_nee_kernel, whose table carries the reverse
 * map in the place of the per-object flags. */
static int mis_enqueue(RtContext* ctx, const void* dRays, int n, void* dOut)
{
    if (int rc = nee_refresh_table(ctx, "rt_mis_trace")) return rc;
    void (*kern)(const KArgs, const float4*, int, float4*, const rtk::NeeTable, const uint32_t*) = RT_SCENE_KERNEL(ctx, rtk::rt_radiance_nee_kernel, true);
    const char* const d = (const char*)ctx->dLightTable;
    rtk::NeeTable lt;
    lt.entries = (const float4*)(d + ctx->lightLayout.entries);
    lt.cdf = (const float*)(d + ctx->lightLayout.cdf);
    lt.inTable = (const uint32_t*)ctx->dLightMap; /* (rt_mis_launch.h: the objects' records, the triangle words behind them) */
    lt.n = ctx->lightSpheres + ctx->lightTriangles;
    return path_enqueue(ctx, SIDE_MIS, RT_SUSPEND_NUM /* (unused: both walks of the pass run to completion) */, n, kern, (const float4*)dRays, n, (float4*)dOut, lt,
                        (const uint32_t*)ctx->dUnitTri);
}

/* ---- the host form and the buffer form of the eight ray-batch calls ----------------------------------------------------------------------
 * What tells the three kinds of batch apart: the pass and its enqueue function, the size of a ray's output, the buffer form's name for
 * the output pointer, the host form's word for the output, and whether the pass reads the parameters. */
struct RayBatch {
    int pass;
    int (*enqueue)(RtContext* ctx, const void* dRays, int n, void* dOut);
    size_t outPerRay;
    const char* outName;
    const char* noun;
    bool needParams;
};
static const RayBatch kClosest = {SIDE_QUERY, closest_enqueue, sizeof(RtRayHit), "d_hits", "records", false};
static const RayBatch kOccluded = {SIDE_QUERY, occluded_enqueue, sizeof(uint32_t), "d_occluded", "answers", false};
static const RayBatch kRadiance = {SIDE_RADIANCE, radiance_enqueue, sizeof(RtRadiance), "d_out", "records", true};
static const RayBatch kNee = {SIDE_NEE, nee_enqueue_host, sizeof(RtRadiance), "d_out", "records", true}; /* (two rows: a table error names the call it came from) */
static const RayBatch kNeeBuffers = {SIDE_NEE, nee_enqueue_buffers, sizeof(RtRadiance), "d_out", "records", true};
static const RayBatch kMis = {SIDE_MIS, mis_enqueue, sizeof(RtRadiance), "out", "records", true};

/* what the calls check before they touch the device; *rayBytes and *outBytes: the sizes of the batch (rt_rd::check_batch is
 * rt_qr::check_batch with an RtRadiance per ray) */
static int rays_check(RtContext* ctx, const char* call, const RayBatch& b, const void* rays, int n, const void* out, size_t* rayBytes, size_t* outBytes)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    const char* why = "";
    if (int rc = rt_qr::check_batch(rays, n, out, b.outPerRay, rayBytes, outBytes, &why)) return fail(ctx, rc, "%s: %s", call, why);
    if (!ctx->haveScene) return fail(ctx, RT_ERR_STATE, "%s before rt_upload_scene", call);
    if (b.needParams && !ctx->haveParams) return fail(ctx, RT_ERR_STATE, "%s before rt_set_params", call);
    return RT_OK;
}

static int rays_to_host(RtContext* ctx, const char* call, const RayBatch& b, const void* rays, int n, void* out)
{
    size_t rayBytes = 0, outBytes = 0;
    int rc = rays_check(ctx, call, b, rays, n, out, &rayBytes, &outBytes);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RT_FLUSH(ctx);
    SidePass& sp = ctx->side[b.pass];
    if ((rc = side_settle(ctx, sp, call))) return rc;
    if (n == 0) return RT_OK;
    if ((rc = grow_scratch(ctx, &ctx->dRays, &ctx->raysBytes, rayBytes))) return rc;
    if ((rc = grow_scratch(ctx, &ctx->dRayOut, &ctx->rayOutBytes, outBytes))) return rc;
    hipStream_t st = joined(ctx);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->dRays, rays, rayBytes, hipMemcpyHostToDevice, st));
    if ((rc = b.enqueue(ctx, ctx->dRays, n, ctx->dRayOut))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(joined(ctx)));
    unsigned long long fired = 0;
    if ((rc = side_fired(ctx, sp, &fired))) return rc;
    if (fired) return fail(ctx, RT_ERR_HIP, "%s: the traversal watchdog fired %llu times in this pass: walks were cut short, the %s are not valid "
                           "(the context's images are not affected)", call, fired, b.noun);
    HIP_TRY(ctx, hipMemcpy(out, ctx->dRayOut, outBytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

static int rays_to_device(RtContext* ctx, const char* call, const RayBatch& b, const void* d_rays, int n, void* d_out)
{
    size_t rayBytes = 0, outBytes = 0;
    int rc = rays_check(ctx, call, b, d_rays, n, d_out, &rayBytes, &outBytes);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n > 0) { /* the kernel reads and writes through these pointers */
        if ((rc = check_device_range(ctx, call, "d_rays", d_rays, rayBytes))) return rc;
        if ((rc = check_device_range(ctx, call, b.outName, d_out, outBytes))) return rc;
    }
    RT_FLUSH(ctx);
    SidePass& sp = ctx->side[b.pass];
    if ((rc = side_settle(ctx, sp, call))) return rc;
    if (n == 0) return RT_OK;
    if ((rc = b.enqueue(ctx, d_rays, n, d_out))) return rc;
    sp.unreported = true;
    return RT_OK;
}

int rt_query_closest(RtContext* ctx, const RtRay* rays, int n, RtRayHit* hits) { return rays_to_host(ctx, "rt_query_closest", kClosest, rays, n, hits); }
int rt_query_closest_buffers(RtContext* ctx, const void* d_rays, int n, void* d_hits) { return rays_to_device(ctx, "rt_query_closest_buffers", kClosest, d_rays, n, d_hits); }
int rt_query_occluded(RtContext* ctx, const RtRay* rays, int n, uint32_t* occluded) { return rays_to_host(ctx, "rt_query_occluded", kOccluded, rays, n, occluded); }
int rt_query_occluded_buffers(RtContext* ctx, const void* d_rays, int n, void* d_occluded) { return rays_to_device(ctx, "rt_query_occluded_buffers", kOccluded, d_rays, n, d_occluded); }
int rt_radiance_trace(RtContext* ctx, const RtPathRay* rays, int n, RtRadiance* out) { return rays_to_host(ctx, "rt_radiance_trace", kRadiance, rays, n, out); }
int rt_radiance_trace_buffers(RtContext* ctx, const void* d_rays, int n, void* d_out) { return rays_to_device(ctx, "rt_radiance_trace_buffers", kRadiance, d_rays, n, d_out); }
int rt_nee_trace(RtContext* ctx, const RtPathRay* rays, int n, RtRadiance* out) { return rays_to_host(ctx, "rt_nee_trace", kNee, rays, n, out); }
int rt_nee_trace_buffers(RtContext* ctx, const void* d_rays, int n, void* d_out) { return rays_to_device(ctx, "rt_nee_trace_buffers", kNeeBuffers, d_rays, n, d_out); }

int rt_nee_light_count(RtContext* ctx, int* n_sphere_emitters, int* n_triangle_emitters)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    if (!ctx->haveScene) return fail(ctx, RT_ERR_STATE, "rt_nee_light_count before rt_upload_scene");
    RT_FLUSH(ctx); /* (the upload goes through the render stream, behind the frames held back) */
    if (int rc = nee_refresh_table(ctx, "rt_nee_light_count")) return rc;
    if (n_sphere_emitters) *n_sphere_emitters = ctx->lightSpheres;
    if (n_triangle_emitters) *n_triangle_emitters = ctx->lightTriangles;
    return RT_OK;
}

int rt_debug_light_table(const RtModel* models, int n_models, const RtTriangle* triangles, int n_triangles, const RtSphere* spheres, int n_spheres,
                         RtLightTableDump* out)
{
    const char* why = "";
    const int rc = rt_lt::dump(models, n_models, triangles, n_triangles, spheres, n_spheres, out, &why);
    return rc ? fail(nullptr, rc, "rt_debug_light_table: %s", why) : RT_OK;
}

void rt_debug_light_table_free(RtLightTableDump* d) { rt_lt::dump_free(d); }

/* include/rt_mis.h: the descriptor first — nothing is touched before it is known to be this library's — then the host or the device
 * form of the ray-batch calls above */
int rt_mis_trace(const RtMisBatch* batch)
{
    if (!batch) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_mis_trace: null descriptor");
    if (batch->struct_size != sizeof(RtMisBatch)) /* (a foreign layout: nothing else of it is read) */
        return fail(nullptr, RT_ERR_INVALID_ARG, "rt_mis_trace: struct_size is %u, this library's RtMisBatch has %zu bytes", batch->struct_size, sizeof(RtMisBatch));
    RtContext* const ctx = batch->ctx; /* (null: the text goes to the global message) */
    if (batch->reserved != 0) return fail(ctx, RT_ERR_INVALID_ARG, "rt_mis_trace: reserved must be 0");
    if (batch->memory > RT_MIS_DEVICE) return fail(ctx, RT_ERR_INVALID_ARG, "rt_mis_trace: memory is %u: RT_MIS_HOST (0) or RT_MIS_DEVICE (1)", batch->memory);
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_mis_trace: null context");
    if (batch->memory == RT_MIS_DEVICE) return rays_to_device(ctx, "rt_mis_trace", kMis, batch->rays, batch->n, batch->out);
    return rays_to_host(ctx, "rt_mis_trace", kMis, batch->rays, batch->n, batch->out);
}

int rt_debug_light_map(const RtModel* models, int n_models, const RtTriangle* triangles, int n_triangles, const RtSphere* spheres, int n_spheres, RtLightMapDump* out)
{
    if (!out) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_debug_light_map: null output");
    memset(out, 0, sizeof(*out));
    const char* why = "";
    try {
        rt_lt::LightTable t;
        if (const int rc = rt_lt::build(models, n_models, reinterpret_cast<const float*>(triangles), sizeof(RtTriangle) / sizeof(float), n_triangles, spheres, n_spheres, t, &why))
            return fail(nullptr, rc, "rt_debug_light_map: %s", why);
        rt_lt::LightMap map;
        rt_lt::build_map(t, models, n_models, n_triangles, n_spheres, map);
        out->objects = (uint32_t*)malloc(map.objects.size() ? map.objects.size() * sizeof(uint32_t) : 1);
        out->triangles = (uint32_t*)malloc(map.triangles.size() ? map.triangles.size() * sizeof(uint32_t) : 1);
        if (!out->objects || !out->triangles) {
            rt_debug_light_map_free(out);
            return fail(nullptr, RT_ERR_OOM, "rt_debug_light_map: out of host memory");
        }
        if (!map.objects.empty()) memcpy(out->objects, map.objects.data(), map.objects.size() * sizeof(uint32_t));
        if (!map.triangles.empty()) memcpy(out->triangles, map.triangles.data(), map.triangles.size() * sizeof(uint32_t));
        out->n_objects = (int32_t)map.objects.size();
        out->n_triangle_words = (int32_t)map.triangles.size();
        out->n_entries = (int32_t)t.entries.size();
    } catch (const std::bad_alloc&) {
        rt_debug_light_map_free(out);
        return fail(nullptr, RT_ERR_OOM, "rt_debug_light_map: out of host memory");
    }
    return RT_OK;
}

void rt_debug_light_map_free(RtLightMapDump* d)
{
    if (!d) return;
    free(d->objects);
    free(d->triangles);
    memset(d, 0, sizeof(*d));
}

} /* extern "C" */

/* ---- rt_gather_rccl's kernel (rt_multi.hip): rank `part`'s packed rows, `rows` of them at `src`, into their global rows of the image
 * at `dst`, on `st`.  Returns the launch's error. */
hipError_t unpack_strips_enqueue(RtContext* ctx, hipStream_t st, const void* src, void* dst, int W, int rows, int stripRows, int part, int parts)
{
    size_t n = (size_t)rows * W;
    int blocks = (int)((n + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(rtk::rt_unpack_strips_kernel, dim3(blocks), dim3(256), 0, st, (const float4*)src, (float4*)dst, W, rows, stripRows, part, parts);
    return hipGetLastError();
}
