/*
 * rt_context.hip — the C ABI of libraytrace_hip.so (include/rt_abi.h): context,
 * scene validation + re-layout for HBM, render-target ownership, launches.
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
#include <dlfcn.h>
#include <sys/mman.h>

#include <cmath>
#include <string>
#include <vector>

#include <algorithm>
#include <chrono>
#include <mutex>

#include "rt_kernels.h"
#include "../../include/rt_cost.h"
#include "../../include/rt_primary.h"
#include "../../include/rt_held_back.h"
#include "../../include/rt_tile_cand.h"
#include "../../include/rt_aov.h"
#include "../../include/rt_denoise.h"
#include "../../include/rt_reproject.h"
#include "../../include/rt_variance.h"
#include "../../include/rt_adaptive.h"
#include "../../include/rt_motion.h"
#include "../../include/rt_query.h"
#include "../../include/rt_radiance.h"
#include "../../include/rt_nee.h"
#include "../../include/rt_mis.h"

#include "rt_denoise_launch.h"
#include "rt_denoise_math.h"
#include "rt_reproject_launch.h"
#include "rt_variance_launch.h"
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
#define RT_VERSION_STRING "raytrace_hip gfx950 abi=1"

static thread_local char g_err[512] = "";

struct RtContext;
struct LaunchJob;
/* The runtime of rt_launch_order.h: its nine events on the context's two render streams, and the kernels a launch's steps enqueue
 * (defined with the launch path, below launch_frames' helpers). */
struct HipOrder final : rt_order::Backend {
    RtContext* ctx = nullptr;
    hipEvent_t ev[rt_order::EVENT_COUNT] = {};
    LaunchJob* job = nullptr; /* the launch LaunchOrder::run is issuing */
    hipStream_t stream(int s) const;
    int record(rt_order::Event e, int s) override;
    int wait(int s, rt_order::Event e) override;
    int sort(int s, int target) override;
    int trace(int s, int part, int parts) override;
    int accumulate(int s) override;
};

/* A side pass — a launch that traces outside the render launches, with a counter slot of its own (see "the side passes" above
 * rt_render_aov).  The context has four, in the order rt_synchronize reports them.  words: the slot, RT_COUNTER_FIELDS words made on
 * first use, of which the kernels write the watchdog word alone (the two radiance passes also count their blocks in word 0); unreported: a
 * device-form pass whose watchdog word has not been read back yet; whose / what: the two places where the deferred report differs by
 * pass. */
struct SidePass {
    unsigned long long* words;
    bool unreported;
    const char* whose;
    const char* what;
};
enum { SIDE_AOV, SIDE_QUERY, SIDE_RADIANCE, SIDE_NEE, SIDE_MIS, SIDE_COUNT };

struct RtContext {
    int device = 0;
    hipStream_t ownStream = nullptr;
    hipStream_t stream = nullptr;
    /* Second render stream (see launch_frames): while the context runs on its own stream, every
     * frame is launched as two kernels over disjoint halves of the tiles, one per stream, so that
     * the drain of one kernel overlaps the other instead of idling the chip. */
    hipStream_t sideStream = nullptr;
    bool twoStreams = true; /* RT_TWO_STREAMS=0: one kernel per launch on the main stream */
    char err[512] = {0};

    /* image */
    int W = 0, H = 0;
    int stripRows = 8, partIndex = 0, partCount = 1;
    int localRows = 0;
    float* ownFrame = nullptr;
    float* ownAccum = nullptr;
    size_t ownBytes = 0;
    float* boundFrame = nullptr;
    float* boundAccum = nullptr;

    /* scene (device) */
    float* dSpheres = nullptr; /* nSpheres x (c, r*r), then nSpheres x (c, |c|^2 - r*r) */
    float sphereBound = 0;     /* max over spheres of |c|^2 + r*r, rounded up */
    DMaterial* dMaterials = nullptr;
    DModel* dModels = nullptr;
    /* the traversal's records, addressed in 16-byte units (rt_layout.h decides where they lie) */
    unsigned char* dPairs = nullptr; /* pair space */
    unsigned char* dTris = nullptr;  /* triangle space; null when the layout keeps the triangles in the pair space (arena) */
    unsigned char* dNorms = nullptr; /* 12 bytes per unit of the triangle space */
    uint32_t* dUnitTri = nullptr;    /* uploaded triangle index by the unit its record starts at (rt_layout.h, unitTri); null: the dense layout */
    bool arenaLayout = false;
    RtLayout layout;                 /* RT_LAYOUT at rt_create */
    std::string layoutUsed = "dense";
    uint32_t* dBigLeaves = nullptr;
    DFilter* dFilters = nullptr;
    DChunk* dChunks = nullptr;  /* two-level model hierarchy, scenes with more than 64 models */
    int nChunks = 0, nFiltered = 0, extWords = 0;
    float filterMaxOrigin = 0.0f;
    std::vector<RtBVHNode> hRootChildren;
    std::vector<RtSphere> hSpheres; /* per model: the root's two children (for rt_update_models) */
    int nSpheres = 0, nModels = 0, nTris = 0, nPairs = 0;
    bool flatScene = false; /* every model root is a leaf: the FLAT kernel variant applies */
    int stackEntries = 1; /* deepest BVH of the scene = most entries a lane can push */
    int wavesPerGroup = 1; /* the BVH variants' workgroups: waves that share one LDS top-of-tree cache (plan_groups) */
    uint32_t hotUnits = 0; /* units [0, hotUnits) of the pair space are that cache's records */
    uint32_t poolSpinLimit = 1u << 16; /* the chain pool's watchdog (rt_kernels.h, pool_exchange); RT_POOL_FAULT=1 (test hook): 64 polls + the fault bit */
    int poolMinItems = 4; /* RT_POOL_MIN_ITEMS: (tile, frame) items per resident wave a launch needs to run as pooled workgroups (choose_variant) */
    int poolWaves = 1, poolCells = 0; /* the FLAT variant's workgroups: waves that share one LDS chain pool (rt_kernels.h, pool_exchange); poolCells = RT_POOL_CELLS or 0 = no pool */
    uint32_t travLimit = 1u << 20; /* traversal watchdog (rt_kernels.h, traverse): 64 x the steps one ray can take in this scene */
    bool haveScene = false;
    /* scene (host mirrors needed by rt_update_models) */
    std::vector<RtModel> hModels;
    std::vector<uint32_t> hRootCodes;
    std::vector<int32_t> hTriBase; /* per model: first unit of its triangles in the triangle space */
    PrimaryTris primaryTris;       /* FLAT scenes within rt_primary.h's caps: the root leaves' triangles, for the per-launch table of origin constants */
    bool primaryOn = true;         /* RT_PRIMARY=0: the table stays off (A/B runs, tests) */
    int lastPrimaryOn = -1;        /* the table's flag in the most recent trace launch's arguments (rt_debug_primary_table); -1 = none yet */
    /* the per-tile sphere candidates of the all-camera-ray waves (rt_tile_cand.h): one table per render stream (0 main, 1 side), each
     * written (rt_tile_cand_kernel) and read (the trace kernels) on its own stream only, so stream order is all the order they need and no
     * launch in flight sees its table change.  A table is refilled, in front of the trace kernel that reads it, only when the key it was
     * made from — camera block, image, partition, diverge, the spheres themselves — is not the launch's */
    bool tileCandOn = true;        /* RT_TILE_CAND=0: the per-ray pre-test stays (A/B runs, tests) */
    int lastTileCand = -1;         /* whether the most recent trace launch read a table (rt_debug_tile_cand); -1 = none yet */
    bool tileTriOn = true;         /* RT_TILE_TRI=0: the table's triangle half stays off alone: every triangle mask is all ones (A/B runs, tests) */
    bool skySunOn = true;          /* RT_SKY_SUN=0: no launch carries RT_USESKY_SUN_UNSEEN, every miss evaluates the sun (A/B runs, tests) */
    int lastTileTri = -1;          /* whether that launch's table held triangle masks (rt_debug_tile_tri); -1 = none yet */
    uint32_t* dTileCand[2] = {nullptr, nullptr};
    int tileCandTiles = 0;         /* tiles the two tables are sized for; 0 = none */
    bool tileCandValid[2] = {false, false};
    TileCandKey tileCandKey[2];    /* what each stream's table holds */
    bool tileCandWanted = false;   /* the launch fill_args last prepared may read a table ... */
    TileCandKey tileCandWant;      /* ... made from this key */

    /* uniforms */
    RtParams params;
    bool haveParams = false;
    int frame = 1;

    /* counters */
    unsigned long long* dCounters = nullptr;
    unsigned long long* dTileQueue = nullptr;      /* monotonic tile counters of the persistent kernel, one per render stream */
    unsigned long long tileQueueNext[2] = {0, 0};  /* value each counter will have when that stream's next launch starts */
    uint32_t* dTileCost = nullptr;  /* per tile: longest pixel chain (segments per frame) seen so far */
    /* queue position -> tile, longest chain first.  Two buffers: a re-sort writes the one no running kernel reads (the kernels in
     * flight keep the order they were launched with), so it does not have to join the streams */
    uint32_t* dTileOrder[2] = {nullptr, nullptr};
    uint32_t* dTileKey = nullptr;   /* the sort's snapshot of the costs (kernels in flight keep raising them) */
    int orderTiles = 0;             /* tiles the two arrays are sized for; 0 = none */
    int numCUs = 256;
    int occPerCU[16] = {0};
    size_t occBytes[16] = {0};
    bool verbose = false;
    /* rt_render_frame calls that arrive while earlier frames are still executing are held back (at most
     * fuseCap) and leave as ONE fused launch at the next call that needs them (flush_pending) */
    void* dPxCold = nullptr; /* pixel records of the resident waves: 2 launch slots (main / side stream) x pxColdWaves x 2 KB */
    long long pxColdWaves = 0;
    int frameGroupOverride = 0; /* RT_FRAME_GROUP: frames per (tile, frame group) item of fused launches (tuning hook) */
    bool coalesce = true;  /* RT_COALESCE=0: every rt_render_frame launches at once */
    int pending = 0;       /* frames [frame - pending, frame) requested but not launched yet */
    bool holdBack = false; /* RT_HOLD_BACK=1 (test hook): gpu_idle answers "busy", so every eligible rt_render_frame is held back */
    bool fuseFrames = true; /* rt_render_frames(n): up to fuseCap frames per launch (RT_FUSE_FRAMES=0: one launch per frame) */
    int fuseCap = RT_FUSE_MIN;  /* frames per fused launch right now (see RT_FUSE_MIN) */
    bool fuseCapPinned = false; /* RT_FUSE_CAP */
    /* the stop event of each fused launch's trace kernel; ms per frame = (stop - previous launch's stop) / frames once both have passed */
    struct FuseProbe { hipEvent_t start = nullptr, stop = nullptr; int frames = 0; int prev = -1; bool live = false; } fuseProbe[6];
    int fuseLast = -1;
    int gridOverride = 0; /* test hook: force the persistent grid size */
    bool stats = false;
    uint64_t pixelFrames = 0;
    /* pinned staging ring of the per-frame update calls (rt_update_models / rt_update_spheres): the
     * uploads are enqueued on the render stream, no host synchronisation */
    struct Staging { void* host = nullptr; size_t cap = 0; hipEvent_t done = nullptr; bool inFlight = false; };
    Staging staging[24]; /* one animated frame uses up to 8 (rt_update_models 4 + rt_update_spheres 4): three frames in flight */
    int stagingNext = 0;
    uint64_t updateUploads = 0, updateSkips = 0; /* diagnostics: uploads enqueued / calls that changed nothing */
    /* Launch tuner (scheduling only, results do not depend on it): the suspension threshold of the traversal loop has two
     * good values, 3/8 and 4/8 of the entrants, and which one is faster depends on how much of a segment is traversal
     * (config 3: 3/8 by 9 %, config 6: 4/8 by 2 %).  Once 48 frames have been rendered, fused launches of >= 8 frames
     * alternate between them, timed with events that are only polled, never waited for; after 3 samples each the
     * faster stays (RT_SUSPEND=3|4 pins it). */
    struct Tuner {
        int decided = 3;       /* value in use once `done` */
        bool done = false;
        double ms[2] = {0, 0}; /* accumulated ms per frame for suspendNum 3, 4 */
        int n[2] = {0, 0};
        int next = 0;          /* which candidate the next measured launch uses */
        struct Probe { hipEvent_t start = nullptr, stop = nullptr; int cand = 0, frames = 0; bool live = false; } probe[6];
    } tuner;
    /* per-frame colours of a fused launch (rt_device.h, KArgs::staging): two slabs, so that consecutive fused launches
     * can alternate between the context's two streams — launch k+1 starts while launch k drains (launch_frames) */
    float* dStaging[2] = {nullptr, nullptr};
    size_t stagingBytes[2] = {0, 0};
    bool stagingUnavailable = false; /* the slab could not be allocated at this image size: fused launches go out frame by frame (cleared by rt_resize) */
    bool alternateWanted = true;     /* RT_ALTERNATE=0: every fused launch on the main stream (round-3 behaviour) */
    /* where launches run and everything the two render streams wait for across each other (rt_launch_order.h) */
    rt_order::LaunchOrder order;
    HipOrder backend;
    int lastLaunched = 0;            /* frames the last launch_frames call really enqueued (flush_pending rolls back the rest) */
    void* dDisplay = nullptr;  /* scratch of the display pass and of the other host reads, kept between calls (grows on demand) */
    size_t displayBytes = 0;
    /* the side passes (SidePass, above): AOV, ray query, radiance, radiance with direct light sampling */
    SidePass side[SIDE_COUNT] = {
        {nullptr, false, "the AOV pass of an rt_render_aov_to_device, rt_denoise_to_device or rt_reproject_accumulated call (or its centre / moving form)", "records or denoised image"},
        {nullptr, false, "the pass of an rt_query_closest_buffers or rt_query_occluded_buffers call", "records or answers"},
        {nullptr, false, "the pass of an rt_radiance_trace_buffers call", "records"},
        {nullptr, false, "the pass of an rt_nee_trace_buffers call", "records"},
        {nullptr, false, "the pass of a device-form rt_mis_trace call", "records"},
    };
    /* rt_nee (include/rt_nee.h): the light table.  hCorners: the local-space corners of the uploaded triangles, nine floats each, kept
     * because rt_update_models can turn any model into an emitter.  The table is rebuilt from the host mirrors by the first call of
     * rt_nee.h behind an upload or an update that changed something (lightDirty), and its device copy — entries, cdf and per-object
     * flags in one allocation (rt_nee_launch.h, table_bytes) — is uploaded on the render stream, behind the passes that read the old one. */
    std::vector<float> hCorners;
    bool lightDirty = true;
    int lightSpheres = 0, lightTriangles = 0;
    rt_nee::TableBytes lightLayout;
    void* dLightTable = nullptr;
    size_t lightTableBytes = 0;
    /* rt_mis (include/rt_mis.h): the reverse map of that table, from a hit to its entry — an allocation of its own (rt_mis_launch.h,
     * map_bytes: the objects' records, the triangle words behind them), rebuilt and uploaded with the table, on the same stream and behind the same passes */
    void* dLightMap = nullptr;
    size_t lightMapBytes = 0;
    /* rt_render_aov (include/rt_aov.h): the host variant's device records, kept between calls (grows on demand) */
    void* dAovOut = nullptr;
    size_t aovOutBytes = 0;
    /* the host forms of rt_query_* and rt_radiance_trace: their device rays and results, kept between calls (grow on demand).  One pair
     * for both: a host form synchronises before it returns and a buffer form uses the caller's memory, so nothing here is live across
     * calls */
    void* dRays = nullptr;
    size_t raysBytes = 0;
    void* dRayOut = nullptr;
    size_t rayOutBytes = 0;
    /* rt_denoise (include/rt_denoise.h): the filter's two colour images and packed guide image, and the AOV records of the two context
     * calls' internal pass; kept between calls (grow on demand) */
    void* dDnScratch = nullptr;
    size_t dnScratchBytes = 0;
    void* dDnAov = nullptr;
    size_t dnAovBytes = 0;
    /* rt_variance (include/rt_variance.h): the moments image and the snapshot of the sum for this context's rows, momentsBytes each;
     * made and zeroed on first use, dropped by rt_resize (so the next use finds them zeroed again) */
    void* dMoments = nullptr;
    void* dSnapshot = nullptr;
    size_t momentsBytes = 0;
    /* rt_adaptive (include/rt_adaptive.h): the tile errors of the last selection and the current tile list, adTilesTotal entries each,
     * for this context's rows; made on first use, dropped by rt_resize.  The host knows the list's length and pixel count (a selection
     * reads them back, a caller's list is counted here).  The launches over a list draw their queue positions from a counter of their
     * own, which counts on across launches like the render streams' (adQueueNext: its value when the next launch starts). */
    float* dAdTileError = nullptr;
    uint32_t* dAdTiles = nullptr;
    uint32_t* dAdCounts = nullptr;
    long long adTilesTotal = -1; /* what the two arrays are sized for; -1 = none */
    bool adHaveList = false, adHaveErrors = false;
    uint32_t adTilesActive = 0, adPixelsActive = 0;
    unsigned long long* dAdQueue = nullptr;
    unsigned long long adQueueNext = 0;
    hipEvent_t evStart = nullptr, evStop = nullptr;
    double gpuMs = 0;
    int timerState = 0; /* 0 idle, 1 begun, 2 ended (elapsed not yet read) */
};

static int fail(RtContext* ctx, int status, const char* fmt, ...)
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

#define HIP_TRY(ctx, call)                                                                          \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return fail(ctx, e_ == hipErrorOutOfMemory ? RT_ERR_OOM : RT_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

/* The main stream, ordered after everything the second render stream has been given.  Every
 * use of the stream other than a render launch goes through here. */
static hipStream_t joined(RtContext* ctx)
{
    (void)ctx->order.join(ctx->backend);
    return ctx->stream;
}

/* The watchdog word: both watchdogs (rt_kernels.h, traverse and pool_exchange) add to word 7 of counter slot 0.  A set word
 * means that walks were cut short or chains dropped, i.e. the accumulated image and the frames rendered since the word was
 * last cleared are wrong.  rt_reset_counters leaves it alone; only rt_reset_accumulation, rt_write_accumulated and rt_resize
 * clear it — stream-ordered behind every launch that could still raise it. */
static const size_t kWatchdogWord = 7;

static int clear_watchdog(RtContext* ctx)
{
    HIP_TRY(ctx, hipMemsetAsync(ctx->dCounters + kWatchdogWord, 0, sizeof(unsigned long long), joined(ctx)));
    return RT_OK;
}

static int watchdog_failure(RtContext* report, const char* call, unsigned long long fired)
{
    return fail(report, RT_ERR_HIP, "%s: a kernel watchdog fired %llu times since the last rt_reset_accumulation / rt_write_accumulated / rt_resize: "
                "walks were cut short or chains dropped, the image is not valid (rt_reset_accumulation clears this)", call, fired);
}

/* Called by every path that hands pixels to a caller, AFTER the synchronise it already performs (8 bytes read back; never on
 * the render path).  `report` receives the message (a multi-context reports through its context 0). */
static int check_watchdog(RtContext* ctx, RtContext* report, const char* call)
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
static int side_fired(RtContext* ctx, const SidePass& sp, unsigned long long* fired)
{
    *fired = 0;
    HIP_TRY(ctx, hipMemcpy(fired, sp.words + kWatchdogWord, sizeof(*fired), hipMemcpyDeviceToHost));
    return RT_OK;
}

/* After a synchronise of the stream: the report of a device-form pass that has not been reported yet */
static int side_report(RtContext* ctx, SidePass& sp, const char* call)
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
static int side_settle(RtContext* ctx, SidePass& sp, const char* call)
{
    if (!sp.unreported) return RT_OK;
    HIP_TRY(ctx, hipStreamSynchronize(joined(ctx)));
    return side_report(ctx, sp, call);
}

static int local_rows_for(int H, int stripRows, int partIndex, int partCount)
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

static void flush_timer(RtContext* ctx)
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
static float* accum_target(const RtContext* ctx) { return ctx->boundAccum ? ctx->boundAccum : ctx->ownAccum; }
static float* frame_target(const RtContext* ctx) { return ctx->boundFrame ? ctx->boundFrame : ctx->ownFrame; }
static float* image_target(const RtContext* ctx, int use_accumulated) { return use_accumulated ? accum_target(ctx) : frame_target(ctx); }

/* Device scratch that is kept between calls and grows on demand: *buf holds at least `bytes` bytes afterwards */
static int grow_scratch(RtContext* ctx, void** buf, size_t* have, size_t bytes)
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
static int check_device_range(RtContext* ctx, const char* call, const char* what, const void* p, size_t bytes)
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

static bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    return (const char*)a < (const char*)b + nb && (const char*)b < (const char*)a + na;
}

/* The caller's buffer for this context's rows: exactly rows x W x perPixel bytes, and a pointer where there are bytes — or always
 * (nullIsError: the reads, the display calls and rt_write_accumulated refuse a null pointer even for a part that owns no rows) */
static int check_rows_buffer(RtContext* ctx, const char* call, size_t perPixel, const void* p, size_t bytes, bool nullIsError = false)
{
    const size_t want = (size_t)ctx->localRows * ctx->W * perPixel;
    if (bytes != want || (!p && (bytes || nullIsError)))
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: need exactly %zu bytes (%d rows x %d x %zu), got %zu%s", call, want, ctx->localRows, ctx->W, perPixel, bytes,
                    p ? "" : " and a null pointer");
    return RT_OK;
}

/* d_rgba of a *_to_device image call, `bytes` bytes: device memory that does not overlap `other` (named `otherName`; nullptr: no such
 * test) — or, without bytes, a pointer that is aligned all the same */
static int check_image_out(RtContext* ctx, const char* call, const void* d_rgba, size_t bytes, const void* other, const char* otherName)
{
    if (!bytes) return ((uintptr_t)d_rgba & 15) ? fail(ctx, RT_ERR_INVALID_ARG, "%s: d_rgba must be 16-byte aligned", call) : RT_OK;
    if (int rc = check_device_range(ctx, call, "d_rgba", d_rgba, bytes)) return rc;
    if (other && ranges_overlap(d_rgba, bytes, other, bytes)) return fail(ctx, RT_ERR_INVALID_ARG, "%s: d_rgba overlaps %s", call, otherName);
    return RT_OK;
}

/* The passes that look at a pixel's neighbours need every row.  A context that passes this one owns pixels (part 0 of 1 of an image
 * rt_resize accepted) — unless rt_set_partition stored the whole-image partition over a part without rows and its rt_resize then failed
 * in HIP before it recomputed localRows; for that one case the context calls behind this check still handle zero bytes. */
static int check_whole_image(RtContext* ctx, const char* call, const char* who, const char* instead)
{
    if (ctx->partCount > 1)
        return fail(ctx, RT_ERR_STATE, "%s: this context owns part %d of %d of the image; %s needs the whole image (%s)", call, ctx->partIndex, ctx->partCount, who, instead);
    return RT_OK;
}

/* width x height of a *_buffers call.  The limit is the caller's: rt_denoise_buffers admits one pixel less than the reprojection and resolve
 * calls (INT32_MAX / 2 against 1 << 30).  Nothing in rt_denoise.hip's indexing (size_t throughout) asks for that; the limits are kept as they
 * were first written. */
static int check_image_size(RtContext* ctx, const char* call, int width, int height, long long maxPixels)
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
static int stage_upload(RtContext* ctx, void* dst, const void* src, size_t bytes)
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
static int flush_pending(RtContext* ctx)
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
#define RT_FLUSH(ctx)                         \
    do {                                      \
        int frc_ = flush_pending(ctx);        \
        if (frc_ != RT_OK) return frc_;       \
    } while (0)

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

static void free_scene(RtContext* ctx)
{
    hipFree(ctx->dSpheres); ctx->dSpheres = nullptr;
    hipFree(ctx->dMaterials); ctx->dMaterials = nullptr;
    hipFree(ctx->dModels); ctx->dModels = nullptr;
    hipFree(ctx->dPairs); ctx->dPairs = nullptr;
    hipFree(ctx->dTris); ctx->dTris = nullptr;
    hipFree(ctx->dNorms); ctx->dNorms = nullptr;
    hipFree(ctx->dUnitTri); ctx->dUnitTri = nullptr;
    hipFree(ctx->dBigLeaves); ctx->dBigLeaves = nullptr;
    hipFree(ctx->dFilters); ctx->dFilters = nullptr;
    hipFree(ctx->dChunks); ctx->dChunks = nullptr;
    ctx->nChunks = 0;
    ctx->haveScene = false;
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

} /* extern "C" */

/* ---------------------------------------------------------------- scene */

template <typename T>
static int upload_vec(RtContext* ctx, T** dptr, const void* src, size_t count)
{
    size_t bytes = count * sizeof(T);
    HIP_TRY(ctx, hipMalloc(dptr, bytes ? bytes : sizeof(T)));
    if (bytes) HIP_TRY(ctx, hipMemcpy(*dptr, src, bytes, hipMemcpyHostToDevice));
    return RT_OK;
}

/* the filter boxes moved: the chunk boxes (and the spatial clustering) follow, stream-ordered */
static int refresh_chunks(RtContext* ctx, const std::vector<DFilter>& filters)
{
    if (!ctx->nChunks) return RT_OK;
    std::vector<DChunk> chunks;
    int nf = 0, ew = 0;
    make_chunks(filters, chunks, &nf, &ew);
    if ((int)chunks.size() != ctx->nChunks) { /* a model became (un)filterable: the split into chunks changed size — rare, synchronous */
        HIP_TRY(ctx, hipStreamSynchronize(joined(ctx)));
        hipFree(ctx->dChunks);
        ctx->dChunks = nullptr;
        int rc = upload_vec(ctx, &ctx->dChunks, chunks.data(), chunks.size());
        if (rc) return rc;
        ctx->nChunks = (int)chunks.size();
        return RT_OK;
    }
    return stage_upload(ctx, ctx->dChunks, chunks.data(), sizeof(DChunk) * chunks.size());
}

/* the models' matrices or the spheres (the scene extent) moved: the root filter boxes again, from the context's root records, then the chunks */
static int refresh_filters(RtContext* ctx, const RtModel* models, const std::vector<RtSphere>& spheres)
{
    std::vector<DFilter> filters;
    make_filters(models, ctx->nModels, ctx->hRootCodes, ctx->hRootChildren, spheres.data(), (int)spheres.size(), filters, &ctx->filterMaxOrigin);
    {
        const std::vector<DFilter> up = append_filter_pairs(filters);
        if (int rc = stage_upload(ctx, ctx->dFilters, up.data(), sizeof(DFilter) * up.size())) return rc;
    }
    return refresh_chunks(ctx, filters);
}


/* device copy of one scene array: from the host vector, or — `peer` — from the context that already holds it, device to
 * device on this context's stream (xGMI when the devices differ; the caller synchronises the stream) */
template <typename T, typename V>
static int commit_vec(RtContext* ctx, T** dptr, const V& v, T* const* peerPtr, const RtContext* peer)
{
    if (!peer) return upload_vec(ctx, dptr, v.data(), v.size());
    const size_t bytes = v.size() * sizeof(T);
    HIP_TRY(ctx, hipMalloc(dptr, bytes ? bytes : sizeof(T)));
    if (bytes) HIP_TRY(ctx, hipMemcpyPeerAsync(*dptr, ctx->device, *peerPtr, peer->device, bytes, ctx->stream));
    return RT_OK;
}

static int commit_scene(RtContext* ctx, const PreparedScene& ps, const RtContext* peer)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(joined(ctx)));
    free_scene(ctx);
    int rc;
    if ((rc = commit_vec(ctx, &ctx->dSpheres, ps.sph, peer ? &peer->dSpheres : nullptr, peer))) return rc;
    if ((rc = commit_vec(ctx, &ctx->dMaterials, ps.mats, peer ? &peer->dMaterials : nullptr, peer))) return rc;
    if ((rc = commit_vec(ctx, &ctx->dModels, ps.dmodels, peer ? &peer->dModels : nullptr, peer))) return rc;
    if ((rc = commit_vec(ctx, &ctx->dPairs, ps.lay.pairBuf, peer ? &peer->dPairs : nullptr, peer))) return rc;
    if (!ps.lay.arena && (rc = commit_vec(ctx, &ctx->dTris, ps.lay.triBuf, peer ? &peer->dTris : nullptr, peer))) return rc;
    if ((rc = commit_vec(ctx, &ctx->dNorms, ps.lay.normBuf, peer ? &peer->dNorms : nullptr, peer))) return rc;
    if (ps.lay.unitTri.size() && (rc = commit_vec(ctx, &ctx->dUnitTri, ps.lay.unitTri, peer ? &peer->dUnitTri : nullptr, peer))) return rc;
    if ((rc = commit_vec(ctx, &ctx->dBigLeaves, ps.lay.bigLeaves, peer ? &peer->dBigLeaves : nullptr, peer))) return rc;
    ctx->arenaLayout = ps.lay.arena;
    ctx->layoutUsed = ps.lay.used.name();
    if ((rc = commit_vec(ctx, &ctx->dFilters, ps.filters, peer ? &peer->dFilters : nullptr, peer))) return rc;
    if ((rc = commit_vec(ctx, &ctx->dChunks, ps.chunks, peer ? &peer->dChunks : nullptr, peer))) return rc;
    ctx->nChunks = (int)ps.chunks.size();
    ctx->nFiltered = ps.nFiltered;
    ctx->extWords = ps.extWords;
    ctx->filterMaxOrigin = ps.maxOrigin;
    ctx->sphereBound = ps.sphereBound;
    ctx->hRootChildren = ps.rootChildren;
    ctx->hSpheres = ps.hSpheres;
    ctx->nSpheres = (int)ps.hSpheres.size();
    ctx->nModels = (int)ps.hModels.size();
    ctx->nTris = ps.nTris;
    ctx->nPairs = (int)ps.nPairs;
    ctx->hTriBase = ps.lay.triBase;
    {
        const auto& triSpace = ps.lay.arena ? ps.lay.pairBuf : ps.lay.triBuf;
        primary_collect_tris(ps.flat, ps.dmodels.data(), (int)ps.dmodels.size(), triSpace.data(), triSpace.size(), ps.lay.bigLeaves.data(), ps.lay.bigLeaves.size(), ctx->primaryTris);
    }
    ctx->stackEntries = ps.flat ? 0 : ps.maxHeight; /* (the FLAT variant pushes nothing: its LDS is pixel bookkeeping only) */
    ctx->flatScene = ps.flat;
    ctx->hotUnits = ps.flat ? 0u : ps.lay.hotUnits;
    {   /* one ray, one segment: every model once (a step each), every pair and every leaf of its tree at most once — and the same tree once
         * per model that uses it.  64 lanes, one step of one lane per iteration at least; the factor 2 is slack, not arithmetic. */
        const unsigned long long steps = (unsigned long long)ps.hModels.size() * (2ull * ps.nPairs + 2ull) + 16ull;
        const unsigned long long lim = 2ull * 64ull * steps;
        ctx->travLimit = lim > 0x7fffffffull ? 0x7fffffffu : (uint32_t)lim;
        if (const char* e = getenv("RT_TRAV_LIMIT")) ctx->travLimit = (uint32_t)strtoul(e, nullptr, 10); /* test hook: make the watchdog fire */
    }
    ctx->wavesPerGroup = ctx->hotUnits ? ps.wavesPerGroup : 1;
    {   /* the FLAT variant's chain pool (rt_kernels.h, pool_exchange): 16-wave workgroups (two per CU at the variant's 8 waves per SIMD), two
         * queues of 64 cells of 128 bytes — 17 KB of the workgroup's 70 KB.  RT_POOL=0: single-wave workgroups without a pool (rounds 1-5);
         * RT_POOL_WAVES: A/B runs and tests */
        int on = 1, waves = RT_MAX_WAVES_PER_GROUP_FLAT;
        if (const char* e = getenv("RT_POOL")) on = atoi(e);
        if (const char* e = getenv("RT_POOL_WAVES")) waves = atoi(e);
        if (waves < 1) waves = 1;
        if (waves > RT_MAX_WAVES_PER_GROUP_FLAT) waves = RT_MAX_WAVES_PER_GROUP_FLAT;
        const bool pooled = ps.flat && on;
        ctx->poolWaves = pooled ? waves : 1;
        ctx->poolCells = pooled ? (int)RT_POOL_CELLS : 0;
    }
    ctx->hModels = ps.hModels;
    ctx->hRootCodes = ps.rootCodes;
    try {
        ctx->hCorners.resize((size_t)ps.nTris * 9); /* (ps.srcTris: the caller's array, alive for the upload call this runs in) */
    } catch (const std::bad_alloc&) {
        return fail(ctx, RT_ERR_OOM, "rt_upload_scene: out of host memory keeping the triangles' corners");
    }
    for (size_t k = 0; k < (size_t)ps.nTris; k++) memcpy(&ctx->hCorners[9 * k], ps.srcTris[k].posA, 36);
    ctx->lightDirty = true;
    ctx->haveScene = true;
    ctx->tuner.done = getenv("RT_SUSPEND") != nullptr; /* RT_SUSPEND=3|4 pins the threshold (tests, A/B runs) */
    ctx->tuner.decided = ctx->tuner.done ? atoi(getenv("RT_SUSPEND")) : 3;
    if (ctx->tuner.decided < 1 || ctx->tuner.decided > 7) ctx->tuner.decided = 3;
    ctx->tuner.ms[0] = ctx->tuner.ms[1] = 0;
    ctx->tuner.n[0] = ctx->tuner.n[1] = 0;
    ctx->tuner.next = 0;
    for (auto& pr : ctx->tuner.probe) pr.live = false;
    return RT_OK;
}

extern "C" {

int rt_upload_scene(RtContext* ctx, const RtModel* models, int n_models, const RtTriangle* triangles, int n_triangles,
                    const RtBVHNode* nodes, int n_nodes, const RtSphere* spheres, int n_spheres)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    RT_FLUSH(ctx);
    PreparedScene ps;
    const auto t0 = std::chrono::steady_clock::now();
    int rc = prepare_scene(models, n_models, triangles, n_triangles, nodes, n_nodes, spheres, n_spheres, ps);
    if (rc) return fail(ctx, rc, "%s", ps.error.c_str());
    const auto t1 = std::chrono::steady_clock::now();
    rc = commit_scene(ctx, ps, nullptr);
    if (getenv("RT_DEBUG_UPLOAD"))
        fprintf(stderr, "[rt] rt_upload_scene: prepare %.2f ms, commit %.2f ms (%d triangles, %zu node pairs)\n",
                std::chrono::duration<double, std::milli>(t1 - t0).count(),
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count(), n_triangles, ps.nPairs);
    return rc;
}

int rt_validate_scene(const RtModel* models, int n_models, const RtTriangle* triangles, int n_triangles,
                      const RtBVHNode* nodes, int n_nodes, const RtSphere* spheres, int n_spheres, RtSceneInfo* out_info)
{
    PreparedScene ps;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = prepare_scene(models, n_models, triangles, n_triangles, nodes, n_nodes, spheres, n_spheres, ps);
    if (rc) fail(nullptr, rc, "%s", ps.error.c_str());
    if (out_info) {
        memset(out_info, 0, sizeof(*out_info));
        out_info->prepare_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (rc == RT_OK) {
            out_info->n_pairs = (int32_t)ps.nPairs;
            out_info->max_height = ps.maxHeight;
            out_info->flat = ps.flat ? 1 : 0;
            out_info->n_filtered = ps.nFiltered;
        }
    }
    return rc;
}

int rt_debug_layout(const RtModel* models, int n_models, const RtTriangle* triangles, int n_triangles,
                    const RtBVHNode* nodes, int n_nodes, const char* layout, RtLayoutDump* out)
{
    if (!out) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_debug_layout: null output");
    memset(out, 0, sizeof(*out));
    PreparedScene ps;
    const int rc = prepare_scene(models, n_models, triangles, n_triangles, nodes, n_nodes, nullptr, 0, ps, layout);
    if (rc) return fail(nullptr, rc, "%s", ps.error.c_str());
    auto take = [](PodVec<unsigned char>& v, unsigned char** p, size_t* n) { *p = v.p; *n = v.n; v.p = nullptr; v.n = 0; };
    take(ps.lay.pairBuf, &out->pair_space, &out->pair_bytes);
    take(ps.lay.triBuf, &out->tri_space, &out->tri_bytes);
    take(ps.lay.normBuf, &out->norm_space, &out->norm_bytes);
    auto dup = [](const void* src, size_t bytes) { void* q = malloc(bytes ? bytes : 1); if (q && bytes) memcpy(q, src, bytes); return q; };
    out->n_big_leaves = ps.lay.bigLeaves.size() / 2;
    out->big_leaves = (uint32_t*)dup(ps.lay.bigLeaves.data(), ps.lay.bigLeaves.size() * 4);
    out->root_codes = (uint32_t*)dup(ps.lay.rootCodes.data(), ps.lay.rootCodes.size() * 4);
    out->tri_base = (int32_t*)dup(ps.lay.triBase.data(), ps.lay.triBase.size() * 4);
    out->n_models = n_models;
    out->arena = ps.lay.arena ? 1 : 0;
    snprintf(out->used, sizeof(out->used), "%s", ps.lay.used.name().c_str());
    return RT_OK;
}

void rt_debug_layout_free(RtLayoutDump* d)
{
    if (!d) return;
    free(d->pair_space); free(d->tri_space); free(d->norm_space); free(d->big_leaves); free(d->root_codes); free(d->tri_base);
    memset(d, 0, sizeof(*d));
}

int rt_update_models(RtContext* ctx, const RtModel* models, int n_models)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    if (!ctx->haveScene) return fail(ctx, RT_ERR_STATE, "rt_update_models before rt_upload_scene");
    if (n_models != ctx->nModels || (n_models && !models)) return fail(ctx, RT_ERR_INVALID_ARG, "rt_update_models: model count changed (%d != %d)", n_models, ctx->nModels);
    if (n_models == 0) return RT_OK;
    /* RCM:192-204 runs every frame; in a static scene nothing changed: no device work at all */
    if (memcmp(models, ctx->hModels.data(), sizeof(RtModel) * (size_t)n_models) == 0) {
        ctx->updateSkips++;
        return RT_OK;
    }
    RT_FLUSH(ctx); /* frames held back were requested with the old models */
    std::vector<DModel> dmodels(n_models);
    std::vector<DMaterial> mats(n_models);
    bool matricesChanged = false;
    for (int i = 0; i < n_models; i++) {
        if (models[i].nodeOffset != ctx->hModels[i].nodeOffset || models[i].triOffset != ctx->hModels[i].triOffset)
            return fail(ctx, RT_ERR_INVALID_ARG, "rt_update_models: model %d changed its BVH offsets; re-upload the scene", i);
        pack_model(models[i], ctx->hRootCodes[i], ctx->hTriBase[i], dmodels[i]);
        pack_material(models[i].material, mats[i]);
        if (memcmp(models[i].worldToLocal, ctx->hModels[i].worldToLocal, sizeof(models[i].worldToLocal)) != 0 ||
            memcmp(models[i].localToWorld, ctx->hModels[i].localToWorld, sizeof(models[i].localToWorld)) != 0)
            matricesChanged = true;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    /* stream-ordered: lands after the frames already enqueued, before the next launch */
    int rc;
    /* (a failure from here on may leave device memory ahead of the host mirrors the table of origin constants is built from:
     * the table then stays off until the next rt_upload_scene — rt_primary.h) */
    if ((rc = stage_upload(ctx, ctx->dModels, dmodels.data(), sizeof(DModel) * n_models))) { ctx->primaryTris.usable = false; return rc; }
    if ((rc = stage_upload(ctx, ctx->dMaterials + ctx->nSpheres, mats.data(), sizeof(DMaterial) * n_models))) { ctx->primaryTris.usable = false; return rc; }
    if (matricesChanged) { /* the world-space root filter boxes depend on the matrices only */
        if ((rc = refresh_filters(ctx, models, ctx->hSpheres))) { ctx->primaryTris.usable = false; return rc; }
    }
    ctx->hModels.assign(models, models + n_models);
    ctx->lightDirty = true;
    return RT_OK;
}

int rt_update_spheres(RtContext* ctx, const RtSphere* spheres, int n_spheres)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    if (!ctx->haveScene) return fail(ctx, RT_ERR_STATE, "rt_update_spheres before rt_upload_scene");
    if (n_spheres != ctx->nSpheres || (n_spheres && !spheres)) return fail(ctx, RT_ERR_INVALID_ARG, "rt_update_spheres: sphere count changed");
    if (n_spheres == 0) return RT_OK;
    if (memcmp(spheres, ctx->hSpheres.data(), sizeof(RtSphere) * (size_t)n_spheres) == 0) {
        ctx->updateSkips++;
        return RT_OK;
    }
    RT_FLUSH(ctx);
    std::vector<float> sph;
    float bound = 0.0f;
    pack_spheres(spheres, n_spheres, sph, &bound);
    std::vector<DMaterial> mats(n_spheres);
    for (int i = 0; i < n_spheres; i++) pack_material(spheres[i].material, mats[i]);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc;
    /* (the bound and the mirror change together with the device records; a failure after the first upload leaves the table of origin
     * constants off until the next rt_upload_scene, as in rt_update_models) */
    if ((rc = stage_upload(ctx, ctx->dSpheres, sph.data(), sph.size() * 4))) { ctx->primaryTris.usable = false; return rc; }
    ctx->sphereBound = bound;
    if ((rc = stage_upload(ctx, ctx->dMaterials, mats.data(), sizeof(DMaterial) * n_spheres))) { ctx->primaryTris.usable = false; return rc; }
    ctx->hSpheres.assign(spheres, spheres + n_spheres);
    ctx->lightDirty = true;
    if (ctx->nModels) { /* the filter margins scale with the scene extent, which includes the spheres */
        if ((rc = refresh_filters(ctx, ctx->hModels.data(), ctx->hSpheres))) return rc;
    }
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

extern "C" {

static int check_renderable(RtContext* ctx)
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

/* ---- rt_adaptive_* (include/rt_adaptive.h): tile selection and the frames of a tile list ---------------------------------------
 * The kernels of the selection and of the list's accumulate step are rt_adaptive.hip's (rt_ad::enqueue_*); the frames themselves are the
 * production trace kernel choose_variant picks, launched over the list: ONE kernel on the joined main stream, whose queue position q is
 * entry q of the list (tileOrder = the list, orderOffset / orderStride = 0 / 1), launchItems from rt_plan::plan_part with tiles = the
 * list's length, tileCost = null (the cost records that order the normal launches are not skewed by partial frames), the main stream's
 * pixel-record slot and staging slab (stream order), and a tile counter of its own.  ctx->order sees a join and nothing else; the
 * tuner and the fuse probes are not touched. */
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

/* Frames frame0 ... frame0 + nFrames - 1 of the current (non-empty) list: one trace kernel and, for nFrames > 1, the list's accumulate
 * step.  *unstaged = true (and nothing enqueued) when nFrames > 1 and there is no staging slab for them. */
static int adaptive_launch(RtContext* ctx, int frame0, int nFrames, bool* unstaged)
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

} /* extern "C" */

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

extern "C" {

/* ---- rt_render_aov / rt_render_aov_to_device (include/rt_aov.h): what camera ray 0 of a frame finds, per pixel -------------
 * The side pass of rt_aov_kernel: KArgs as for frame `frame`, the tiles strided over the resident waves.  frame == RT_AOV_CENTRE (0)
 * selects the pixel-centre ray of include/rt_motion.h, which reads nothing of a frame: the KArgs are then those of frame 1. */
static int aov_enqueue(RtContext* ctx, int frame, void* dOut)
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

/* ------------------------------------------------------------------------------------------
 * Several GPUs from one host process: n contexts with cyclic 8-row strips, gather at readback.
 * ---------------------------------------------------------------------------------------- */
struct RtMulti {
    std::vector<RtContext*> ctx;
    /* pinned staging of the gather: every context's packed rows, copied device -> host concurrently */
    void* pinned = nullptr;
    size_t pinnedBytes = 0;
    double lastGatherMs = 0;
    /* peer access between the distinct devices of this multi-context (hipDeviceCanAccessPeer / hipDeviceEnablePeerAccess at
     * creation): peerPairs = ordered pairs of distinct devices, peerEnabled = of those, the pairs with direct access (xGMI or
     * PCIe P2P).  Without it hipMemcpyPeerAsync still works — the runtime stages through host memory — only slower. */
    int peerPairs = 0, peerEnabled = 0;
};

/* launch what every context holds back BEFORE waiting for any of them: a per-context synchronise in a loop would start
 * device i+1's held frames only after device i has finished */
static int multi_flush_all(RtMulti* m)
{
    for (RtContext* c : m->ctx) {
        int rc = rt_flush(c);
        if (rc != RT_OK) return rc;
    }
    return RT_OK;
}

/* wait for whatever the contexts' streams hold (error paths of the gathers: nothing may still be writing into the caller's
 * buffer when an error is returned) */
static void multi_drain(RtMulti* m)
{
    for (RtContext* c : m->ctx) {
        if (hipSetDevice(c->device) != hipSuccess) { (void)hipGetLastError(); continue; }
        (void)hipStreamSynchronize(joined(c));
        (void)hipGetLastError();
    }
}

int rt_create_multi(const int* device_ids, int n_devices, RtMulti** out)
{
    if (!out) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_create_multi: out is null");
    *out = nullptr;
    if (!device_ids || n_devices <= 0) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_create_multi: no devices");
    RtMulti* m = new RtMulti();
    for (int i = 0; i < n_devices; i++) {
        RtContext* c = nullptr;
        int rc = rt_create(device_ids[i], &c);
        if (rc == RT_OK) rc = rt_set_partition(c, 8, i, n_devices);
        if (rc != RT_OK) {
            if (c) rt_destroy(c);
            rt_destroy_multi(m);
            return rc;
        }
        m->ctx.push_back(c);
    }
    /* direct device-to-device copies (scene replication at upload, rt_gather_*_to_device) need peer access enabled in both
     * directions; "already enabled" is fine, "cannot" leaves the pair on the runtime's host-staged path */
    for (int i = 0; i < n_devices; i++)
        for (int j = 0; j < n_devices; j++) {
            const int di = m->ctx[i]->device, dj = m->ctx[j]->device;
            if (di == dj) continue;
            bool seen = false; /* the same pair listed twice (virtual shards on one device list) counts once */
            for (int i2 = 0; i2 < n_devices && !seen; i2++)
                for (int j2 = 0; j2 < n_devices && !seen; j2++)
                    if ((i2 < i || (i2 == i && j2 < j)) && m->ctx[i2]->device == di && m->ctx[j2]->device == dj) seen = true;
            if (seen) continue;
            m->peerPairs++;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, di, dj) != hipSuccess) { (void)hipGetLastError(); can = 0; }
            if (!can) continue;
            if (hipSetDevice(di) != hipSuccess) { (void)hipGetLastError(); continue; }
            const hipError_t e = hipDeviceEnablePeerAccess(dj, 0);
            if (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) m->peerEnabled++;
            (void)hipGetLastError();
        }
    *out = m;
    return RT_OK;
}

/* How device-to-device copies between this multi-context's GPUs travel: 2 = every pair of distinct devices has direct peer access
 * (xGMI / PCIe P2P), 1 = some pairs, 0 = none (the runtime stages through host memory), -1 = one device only (nothing to copy
 * between devices).  *pairs / *enabled (optional) receive the counts. */
int rt_multi_peer_access(const RtMulti* m, int* pairs, int* enabled)
{
    if (!m) return RT_ERR_INVALID_ARG;
    if (pairs) *pairs = m->peerPairs;
    if (enabled) *enabled = m->peerEnabled;
    if (m->peerPairs == 0) return -1;
    return m->peerEnabled == m->peerPairs ? 2 : (m->peerEnabled > 0 ? 1 : 0);
}

void rt_destroy_multi(RtMulti* m)
{
    if (!m) return;
    for (RtContext* c : m->ctx) rt_destroy(c);
    if (m->pinned) hipHostFree(m->pinned);
    delete m;
}

int rt_multi_count(const RtMulti* m) { return m ? (int)m->ctx.size() : 0; }
RtContext* rt_multi_context(RtMulti* m, int i) { return (m && i >= 0 && i < (int)m->ctx.size()) ? m->ctx[i] : nullptr; }

#define RT_MULTI_FORWARD(call)                                                 \
    do {                                                                       \
        if (!m) return fail(nullptr, RT_ERR_INVALID_ARG, "null multi context"); \
        for (RtContext* c : m->ctx) {                                          \
            int rc_ = (call);                                                  \
            if (rc_ != RT_OK) return rc_;                                      \
        }                                                                      \
        return RT_OK;                                                          \
    } while (0)

int rt_multi_resize(RtMulti* m, int width, int height) { RT_MULTI_FORWARD(rt_resize(c, width, height)); }
int rt_multi_upload_scene(RtMulti* m, const RtModel* models, int n_models, const RtTriangle* triangles, int n_triangles,
                          const RtBVHNode* nodes, int n_nodes, const RtSphere* spheres, int n_spheres)
{
    /* validated and re-laid out once; context 0 gets it from the host, the others copy context 0's device arrays
     * (hipMemcpyPeerAsync on their own streams: all destinations at once, over xGMI between different devices) */
    if (!m || m->ctx.empty()) return fail(nullptr, RT_ERR_INVALID_ARG, "null multi context");
    int rc = multi_flush_all(m);
    if (rc) return rc;
    PreparedScene ps;
    RtContext* c0 = m->ctx[0];
    if ((rc = prepare_scene(models, n_models, triangles, n_triangles, nodes, n_nodes, spheres, n_spheres, ps))) return fail(c0, rc, "%s", ps.error.c_str());
    if ((rc = commit_scene(c0, ps, nullptr))) return rc;
    const bool peerCopies = getenv("RT_MULTI_PEER_UPLOAD") == nullptr || atoi(getenv("RT_MULTI_PEER_UPLOAD")) != 0;
    for (size_t i = 1; i < m->ctx.size(); i++) {
        rc = commit_scene(m->ctx[i], ps, peerCopies ? c0 : nullptr);
        if (rc != RT_OK && peerCopies) rc = commit_scene(m->ctx[i], ps, nullptr); /* no peer path between the two: from the host */
        if (rc != RT_OK) return rc;
    }
    for (size_t i = 1; i < m->ctx.size(); i++) { /* the copies read context 0's arrays: done before anyone may replace them */
        RtContext* c = m->ctx[i];
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return RT_OK;
}
int rt_multi_update_models(RtMulti* m, const RtModel* models, int n_models) { RT_MULTI_FORWARD(rt_update_models(c, models, n_models)); }
int rt_multi_update_spheres(RtMulti* m, const RtSphere* spheres, int n_spheres) { RT_MULTI_FORWARD(rt_update_spheres(c, spheres, n_spheres)); }
int rt_multi_set_params(RtMulti* m, const RtParams* params) { RT_MULTI_FORWARD(rt_set_params(c, params)); }
int rt_multi_reset_accumulation(RtMulti* m) { RT_MULTI_FORWARD(rt_reset_accumulation(c)); }
int rt_multi_render_frame(RtMulti* m) { RT_MULTI_FORWARD(rt_render_frame(c)); }
int rt_multi_render_frames(RtMulti* m, int n) { RT_MULTI_FORWARD(rt_render_frames(c, n)); }
int rt_multi_synchronize(RtMulti* m)
{
    if (!m) return fail(nullptr, RT_ERR_INVALID_ARG, "null multi context");
    int rc = multi_flush_all(m);
    if (rc) return rc;
    RT_MULTI_FORWARD(rt_synchronize(c));
}
double rt_multi_last_gather_ms(const RtMulti* m) { return m ? m->lastGatherMs : 0.0; }

static int multi_gather(RtMulti* m, float* rgba, size_t bytes, bool accumulated)
{
    if (!m || m->ctx.empty()) return fail(nullptr, RT_ERR_INVALID_ARG, "null multi context");
    RtContext* c0 = m->ctx[0];
    const int W = c0->W, H = c0->H;
    if (!rgba || bytes != (size_t)W * H * 16) return fail(c0, RT_ERR_INVALID_ARG, "rt_gather: bytes %zu != H*W*16 = %zu", bytes, (size_t)W * H * 16);
    const size_t rowBytes = (size_t)W * 16;
    size_t total = 0;
    for (RtContext* c : m->ctx) {
        if (c->W != W || c->H != H) return fail(c0, RT_ERR_STATE, "rt_gather: contexts disagree on the resolution");
        total += (size_t)c->localRows * rowBytes;
    }
    if (m->pinnedBytes < total) {
        if (m->pinned) hipHostFree(m->pinned);
        m->pinned = nullptr;
        m->pinnedBytes = 0;
        HIP_TRY(c0, hipHostMalloc(&m->pinned, total ? total : 16, hipHostMallocDefault));
        m->pinnedBytes = total;
    }
    /* every device's held frames are launched, then every device's tile is on its way to pinned host memory (each on
     * its own stream and its own link), and only then does the host wait — device by device, scattering the tile that
     * has arrived while the others are still in flight */
    int rc = multi_flush_all(m);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    size_t off = 0;
    for (RtContext* c : m->ctx) {
        const size_t n = (size_t)c->localRows * rowBytes;
        if (n) {
            const float* src = image_target(c, accumulated);
            hipError_t e = hipSetDevice(c->device);
            if (e == hipSuccess) e = hipMemcpyAsync((char*)m->pinned + off, src, n, hipMemcpyDeviceToHost, joined(c));
            if (e != hipSuccess) { /* copies already enqueued still write into m->pinned: wait for them before handing the error back */
                multi_drain(m);
                return fail(c, RT_ERR_HIP, "rt_gather: %s", hipGetErrorString(e));
            }
        }
        off += n;
    }
    off = 0;
    for (RtContext* c : m->ctx) {
        const int rows = c->localRows;
        const size_t n = (size_t)rows * rowBytes;
        if (!n) continue;
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        flush_timer(c);
        if ((rc = check_watchdog(c, c0, "rt_gather"))) { /* the later contexts' copies still write into m->pinned */
            multi_drain(m);
            return rc;
        }
        /* packed local rows -> their global rows; a strip's rows are contiguous in both */
        for (int l = 0; l < rows;) {
            const int g = rt_local_to_global_row(c, l);
            int run = c->stripRows - (g % c->stripRows);
            if (run > rows - l) run = rows - l;
            memcpy((char*)rgba + (size_t)g * rowBytes, (const char*)m->pinned + off + (size_t)l * rowBytes, (size_t)run * rowBytes);
            l += run;
        }
        off += n;
    }
    m->lastGatherMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return RT_OK;
}
/* The gather with a DEVICE destination: every context's strips go straight into their global rows of an image on the
 * device of context `root` — device-to-device copies on each source context's own stream (ordered after its frames; xGMI
 * between different GPUs, all sources concurrently), no host memory in between.  For hosts that display or post-process on
 * one of the GPUs. */
static int multi_gather_device(RtMulti* m, int root, void* d_rgba, size_t bytes, bool accumulated)
{
    if (!m || m->ctx.empty()) return fail(nullptr, RT_ERR_INVALID_ARG, "null multi context");
    RtContext* c0 = m->ctx[0];
    if (root < 0 || root >= (int)m->ctx.size()) return fail(c0, RT_ERR_INVALID_ARG, "rt_gather_*_to_device: root %d out of range", root);
    const int W = c0->W, H = c0->H;
    if (!d_rgba || bytes != (size_t)W * H * 16) return fail(c0, RT_ERR_INVALID_ARG, "rt_gather_*_to_device: bytes %zu != H*W*16 = %zu", bytes, (size_t)W * H * 16);
    const size_t rowBytes = (size_t)W * 16;
    const int rootDev = m->ctx[root]->device;
    for (RtContext* c : m->ctx) /* before anything is enqueued */
        if (c->W != W || c->H != H) return fail(c0, RT_ERR_STATE, "rt_gather: contexts disagree on the resolution");
    int rc = multi_flush_all(m);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    for (RtContext* c : m->ctx) {
        const int rows = c->localRows;
        if (!rows) continue;
        const char* src = (const char*)image_target(c, accumulated);
        hipError_t e = hipSetDevice(c->device);
        hipStream_t st = joined(c);
        for (int l = 0; l < rows && e == hipSuccess;) { /* a strip's rows are contiguous in the packed tile and in the image */
            const int g = rt_local_to_global_row(c, l);
            int run = c->stripRows - (g % c->stripRows);
            if (run > rows - l) run = rows - l;
            e = hipMemcpyPeerAsync((char*)d_rgba + (size_t)g * rowBytes, rootDev, src + (size_t)l * rowBytes, c->device, (size_t)run * rowBytes, st);
            l += run;
        }
        if (e != hipSuccess) { /* earlier contexts' copies into the caller's buffer are still in flight: wait before returning */
            multi_drain(m);
            return fail(c, RT_ERR_HIP, "rt_gather_*_to_device: %s", hipGetErrorString(e));
        }
    }
    for (RtContext* c : m->ctx) {
        if (!c->localRows) continue;
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        flush_timer(c);
    }
    for (RtContext* c : m->ctx) /* after every copy into the caller's buffer has completed */
        if (c->localRows && (rc = check_watchdog(c, c0, "rt_gather_*_to_device"))) return rc;
    m->lastGatherMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return RT_OK;
}
int rt_gather_accumulated_to_device(RtMulti* m, int root, void* d_rgba, size_t bytes) { return multi_gather_device(m, root, d_rgba, bytes, true); }
int rt_gather_frame_to_device(RtMulti* m, int root, void* d_rgba, size_t bytes) { return multi_gather_device(m, root, d_rgba, bytes, false); }
int rt_gather_accumulated(RtMulti* m, float* rgba, size_t bytes) { return multi_gather(m, rgba, bytes, true); }
int rt_gather_frame(RtMulti* m, float* rgba, size_t bytes) { return multi_gather(m, rgba, bytes, false); }

/* ---- RCCL, loaded on first use (no link-time dependency): the handful of entry points rt_gather_rccl needs */
namespace {
struct Rccl {
    void* lib = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*CommCount)(void*, int*) = nullptr;
    int (*CommUserRank)(void*, int*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool ok = false;
};
Rccl* rccl()
{
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        const char* names[] = {getenv("RT_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char* n : names) {
            if (!n) continue;
            r.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
            if (r.lib) break;
        }
        if (!r.lib) return;
        r.GroupStart = (int (*)())dlsym(r.lib, "ncclGroupStart");
        r.GroupEnd = (int (*)())dlsym(r.lib, "ncclGroupEnd");
        r.Send = (int (*)(const void*, size_t, int, int, void*, hipStream_t))dlsym(r.lib, "ncclSend");
        r.Recv = (int (*)(void*, size_t, int, int, void*, hipStream_t))dlsym(r.lib, "ncclRecv");
        r.CommCount = (int (*)(void*, int*))dlsym(r.lib, "ncclCommCount");
        r.CommUserRank = (int (*)(void*, int*))dlsym(r.lib, "ncclCommUserRank");
        r.GetErrorString = (const char* (*)(int))dlsym(r.lib, "ncclGetErrorString");
        r.ok = r.GroupStart && r.GroupEnd && r.Send && r.Recv && r.CommCount && r.CommUserRank;
    });
    return &r;
}
} // namespace

int rt_gather_rccl(RtContext* ctx, void* nccl_comm, int root, int use_accumulated, void* d_rgba, size_t bytes)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    RT_FLUSH(ctx);
    if (!nccl_comm) return fail(ctx, RT_ERR_INVALID_ARG, "rt_gather_rccl: null communicator");
    if (ctx->W == 0) return fail(ctx, RT_ERR_STATE, "rt_gather_rccl before rt_resize");
    Rccl* R = rccl();
    if (!R->ok) return fail(ctx, RT_ERR_STATE, "rt_gather_rccl: librccl.so could not be loaded (%s)", R->lib ? "missing symbols" : "dlopen failed; RT_RCCL_LIB names another path");
    int world = 0, rank = -1;
    if (R->CommCount(nccl_comm, &world) != 0 || R->CommUserRank(nccl_comm, &rank) != 0) return fail(ctx, RT_ERR_INVALID_ARG, "rt_gather_rccl: not a communicator");
    if (world != ctx->partCount || rank != ctx->partIndex)
        return fail(ctx, RT_ERR_STATE, "rt_gather_rccl: communicator rank %d of %d, context partition %d of %d", rank, world, ctx->partIndex, ctx->partCount);
    if (root < 0 || root >= world) return fail(ctx, RT_ERR_INVALID_ARG, "rt_gather_rccl: root %d out of range", root);
    const int W = ctx->W, H = ctx->H;
    const bool isRoot = rank == root;
    /* a collective: what only ONE rank can get wrong must not keep it out of the exchange (its peers would block in ncclSend for ever):
     * a root with a bad destination still receives every tile, and says so afterwards (include/rt_abi.h) */
    const bool badDst = isRoot && (!d_rgba || bytes != (size_t)W * H * 16);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = joined(ctx);
    const float* src = image_target(ctx, use_accumulated);
    /* root: one staging area for every rank's packed tile (H rows in all), then one watchdog word per rank, in the display scratch */
    std::vector<size_t> rowOff(world + 1, 0);
    for (int r = 0; r < world; r++) rowOff[r + 1] = rowOff[r] + (size_t)local_rows_for(H, ctx->stripRows, r, world);
    const size_t tileBytes = rowOff[world] * (size_t)W * 16;
    char* staging = nullptr;
    unsigned long long* flags = nullptr;
    if (isRoot) {
        const int rc = grow_scratch(ctx, &ctx->dDisplay, &ctx->displayBytes, tileBytes + (size_t)world * sizeof(unsigned long long));
        if (rc) return rc;
        staging = (char*)ctx->dDisplay;
        flags = (unsigned long long*)(staging + tileBytes);
    }
    auto check = [&](int e, const char* what) -> int {
        if (e == 0) return RT_OK;
        return fail(ctx, RT_ERR_HIP, "rt_gather_rccl: %s: %s", what, R->GetErrorString ? R->GetErrorString(e) : "RCCL error");
    };
    /* every rank sends its tile to root, root receives from every rank — its own included, so that a one-rank communicator runs the
     * same code; one group: the transfers progress together.  Behind its tile each rank sends its watchdog word (a tripped rank still
     * takes part in the exchange: the root learns of it and fails) */
    int rc = check(R->GroupStart(), "ncclGroupStart");
    if (rc) return rc;
    int e = 0;
    if (ctx->localRows) e = R->Send(src, (size_t)ctx->localRows * W * 4, /*ncclFloat32*/ 7, root, nccl_comm, st);
    if (e == 0) e = R->Send(ctx->dCounters + kWatchdogWord, 1, /*ncclUint64*/ 5, root, nccl_comm, st);
    if (isRoot)
        for (int r = 0; r < world && e == 0; r++) {
            const size_t rows = rowOff[r + 1] - rowOff[r];
            if (rows) e = R->Recv(staging + rowOff[r] * (size_t)W * 16, rows * W * 4, 7, r, nccl_comm, st);
            if (e == 0) e = R->Recv(flags + r, 1, 5, r, nccl_comm, st);
        }
    const int eEnd = R->GroupEnd();
    if ((rc = check(e, "ncclSend / ncclRecv"))) return rc;
    if ((rc = check(eEnd, "ncclGroupEnd"))) return rc;
    if (isRoot && !badDst)
        for (int r = 0; r < world; r++) {
            const int rows = (int)(rowOff[r + 1] - rowOff[r]);
            if (!rows) continue;
            size_t n = (size_t)rows * W;
            int blocks = (int)((n + 255) / 256);
            if (blocks > 4096) blocks = 4096;
            hipLaunchKernelGGL(rtk::rt_unpack_strips_kernel, dim3(blocks), dim3(256), 0, st, (const float4*)(staging + rowOff[r] * (size_t)W * 16), (float4*)d_rgba, W, rows,
                               ctx->stripRows, r, world);
            HIP_TRY(ctx, hipGetLastError());
        }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    flush_timer(ctx);
    if ((rc = check_watchdog(ctx, ctx, "rt_gather_rccl"))) return rc;
    if (isRoot) {
        std::vector<unsigned long long> fired(world);
        HIP_TRY(ctx, hipMemcpy(fired.data(), flags, (size_t)world * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (int r = 0; r < world; r++)
            if (fired[r]) {
                char what[64];
                snprintf(what, sizeof(what), "rt_gather_rccl (rank %d of %d)", r, world);
                return watchdog_failure(ctx, what, fired[r]);
            }
    }
    if (badDst) return fail(ctx, RT_ERR_INVALID_ARG, "rt_gather_rccl: bytes %zu != H*W*16 = %zu (the tiles were received and dropped)", bytes, (size_t)W * H * 16);
    return RT_OK;
}

int rt_debug_multi_pending_frames(const RtMulti* m)
{
    if (!m) return RT_ERR_INVALID_ARG;
    int most = 0;
    for (const RtContext* c : m->ctx) most = c->pending > most ? c->pending : most;
    return most;
}

int rt_multi_get_counters(RtMulti* m, RtCounters* out)
{
    if (!m || !out) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_multi_get_counters: null argument");
    memset(out, 0, sizeof(*out));
    {
        int rc = multi_flush_all(m);
        if (rc) return rc;
    }
    for (size_t i = 0; i < m->ctx.size(); i++) {
        RtContext* c = m->ctx[i];
        RtCounters k;
        int rc = rt_get_counters(c, &k);
        if (rc != RT_OK) return i == 0 ? rc : fail(m->ctx[0], rc, "context %zu: %s", i, c->err); /* read through context 0 */
        out->segments += k.segments; out->innerSteps += k.innerSteps; out->leafSteps += k.leafSteps; out->triTests += k.triTests;
        out->sphereTests += k.sphereTests; out->modelVisits += k.modelVisits; out->pixelFrames += k.pixelFrames;
        if (k.gpuMs > out->gpuMs) out->gpuMs = k.gpuMs;
    }
    return RT_OK;
}

} /* extern "C" */
