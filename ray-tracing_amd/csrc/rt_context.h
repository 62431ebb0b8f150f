/*
 * rt_context.h — what the translation units behind the C ABI share: the context, the macros of an entry point and the helpers
 * that more than one unit calls.  Internal: the helpers have hidden visibility, the library exports include/rt_abi.h and no more.
 *     rt_context.hip       context lifetime, the launch path, the side passes — every kernel launch; the one includer of rt_kernels.h
 *     rt_scene_upload.hip  the device half of the scene upload and of the update calls
 *     rt_post.hip          the passes behind the render: denoise, reproject, motion, resolve, variance, adaptive
 *     rt_multi.hip         several GPUs: RtMulti, the gathers, the RCCL loader
 * A helper that one unit alone calls is static in that unit and not declared here.  Of HIP, only the runtime API's types.
 */
#pragma once

#include <hip/hip_runtime_api.h>

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/rt_abi.h"
#include "rt_launch_order.h"
#include "rt_layout.h"
#include "rt_nee_launch.h"
#include "rt_primary.h"
#include "rt_records.h"
#include "rt_tile_cand.h"

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

/* A HIP call of a function that returns a status: a failure ends the function with RT_ERR_OOM or RT_ERR_HIP and the call's text */
#define HIP_TRY(ctx, call)                                                                          \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return fail(ctx, e_ == hipErrorOutOfMemory ? RT_ERR_OOM : RT_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

/* The watchdog word: both watchdogs (rt_kernels.h, traverse and pool_exchange) add to word 7 of counter slot 0.  A set word
 * means that walks were cut short or chains dropped, i.e. the accumulated image and the frames rendered since the word was
 * last cleared are wrong.  rt_reset_counters leaves it alone; only rt_reset_accumulation, rt_write_accumulated and rt_resize
 * clear it — stream-ordered behind every launch that could still raise it. */
static const size_t kWatchdogWord = 7;

/* First thing in every entry point that reads or changes what the frames held back depend on, or hands results to the host */
#define RT_FLUSH(ctx)                         \
    do {                                      \
        int frc_ = flush_pending(ctx);        \
        if (frc_ != RT_OK) return frc_;       \
    } while (0)

struct PreparedScene; /* rt_scene_prep.h */

#pragma GCC visibility push(hidden)
/* rt_context.hip: messages, the joined stream, the frames held back */
int fail(RtContext* ctx, int status, const char* fmt, ...);
hipStream_t joined(RtContext* ctx);
int flush_pending(RtContext* ctx);
void flush_timer(RtContext* ctx);
/* rt_context.hip: the watchdog words */
int watchdog_failure(RtContext* report, const char* call, unsigned long long fired);
int check_watchdog(RtContext* ctx, RtContext* report, const char* call);
int side_fired(RtContext* ctx, const SidePass& sp, unsigned long long* fired);
int side_report(RtContext* ctx, SidePass& sp, const char* call);
int side_settle(RtContext* ctx, SidePass& sp, const char* call);
/* rt_context.hip: targets, scratch, uploads, argument checks */
int local_rows_for(int H, int stripRows, int partIndex, int partCount);
float* accum_target(const RtContext* ctx);
float* image_target(const RtContext* ctx, int use_accumulated);
int grow_scratch(RtContext* ctx, void** buf, size_t* have, size_t bytes);
int stage_upload(RtContext* ctx, void* dst, const void* src, size_t bytes);
int check_device_range(RtContext* ctx, const char* call, const char* what, const void* p, size_t bytes);
bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb);
int check_rows_buffer(RtContext* ctx, const char* call, size_t perPixel, const void* p, size_t bytes, bool nullIsError = false);
int check_image_out(RtContext* ctx, const char* call, const void* d_rgba, size_t bytes, const void* other, const char* otherName);
int check_whole_image(RtContext* ctx, const char* call, const char* who, const char* instead);
int check_image_size(RtContext* ctx, const char* call, int width, int height, long long maxPixels);
int check_renderable(RtContext* ctx);
/* rt_context.hip: the kernel launches the other units ask for */
int aov_enqueue(RtContext* ctx, int frame, void* dOut);
int adaptive_launch(RtContext* ctx, int frame0, int nFrames, bool* unstaged);
hipError_t unpack_strips_enqueue(RtContext* ctx, hipStream_t st, const void* src, void* dst, int W, int rows, int stripRows, int part, int parts);
/* rt_scene_upload.hip */
int commit_scene(RtContext* ctx, const PreparedScene& ps, const RtContext* peer);
void free_scene(RtContext* ctx);
#pragma GCC visibility pop
