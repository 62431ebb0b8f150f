/*
 * rt_launch_plan.h — the arithmetic that sizes a launch, in one module without HIP.
 *
 * rt_context.hip gathers the inputs (scene, context, env switches, the occupancy the runtime reports, measured times), calls these pure
 * functions and copies the results into KArgs / LaunchPlan; tests/test_launch_plan.py checks them on the CPU.  The launch geometry the
 * kernels are compiled with is defined here too (rt_records.h includes this header, rt_device.h through it), so that the host's rules and the kernels cannot
 * disagree about a constant.
 *
 *   what                                  function        used by
 *   BVH workgroups, top-of-tree cache     plan_groups     prepare_scene (once per upload: the layout's cache prefix is sized by it)
 *   filtered models, mask extension       filtering       make_chunks, plan_groups
 *   pooled?, workgroup shape, LDS, slot   launch_shape    choose_variant
 *   pixel-record waves                    record_waves    prepare_records
 *   per-part work split, grid, queue      plan_part       HipOrder::trace
 *   staging slab frames                   slab_frames     prepare_staging
 *   frames per fused launch               fuse_cap        tune_launch; pinned_fuse_cap: RT_FUSE_CAP at rt_create
 *   suspension tuner                      tuner_*         tune_launch
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>

/* functions the kernels call too (include/rt_math.h defines the same macro the same way) */
#ifndef RT_HD
#if defined(__HIPCC__)
#define RT_HD __host__ __device__ __forceinline__
#else
#define RT_HD inline
#endif
#endif

/* ---- launch geometry, shared with the kernels */
#define RT_WAVE 64
#define RT_PIXEL_FIELDS 4
#define RT_MAX_WAVES_PER_GROUP 12      /* the BVH trace kernels' workgroups: up to 12 waves share one LDS top-of-tree cache (rt_kernels.h) */
/* the FLAT trace kernel's workgroups (round 6): up to 16 waves share one LDS CHAIN POOL (rt_kernels.h, pool_exchange): two queues (chains
 * waiting for the sky phase / for the shade phase) of RT_POOL_CELLS cells each (a power of two; 32 measured 10 % slower than 64 on the headline
 * scene, 128 the same as 64: profiles/r06_chain_pool.txt); a cell = RT_POOL_QUADS x 16 bytes of chain state.
 * LDS of a workgroup: [header: RT_POOL_HEADER_DWORDS][seq: 2 x RT_POOL_CELLS dwords][payload: 2 x RT_POOL_QUADS x RT_POOL_CELLS x 16 B][wave regions] */
#define RT_MAX_WAVES_PER_GROUP_FLAT 16
#define RT_POOL_CELLS 64u
#define RT_POOL_QUADS 8u
#define RT_POOL_HEADER_DWORDS 16u
#define RT_POOL_DWORDS (RT_POOL_HEADER_DWORDS + 2u * RT_POOL_CELLS + 2u * RT_POOL_QUADS * RT_POOL_CELLS * 4u)
/* waves per SIMD the register allocator must leave room for (launch_bounds 2nd argument, rt_kernels.h).  Built without the SLP
 * vectoriser (Makefile) the BVH variants need 83 VGPRs: 6 waves = 80 VGPRs costs no spill and is worth 2–7 % per frame
 * (7 waves: 30 spilled dwords, slower); the FLAT variant fits 8 waves = 64 VGPRs (−9 % on config 2). */
#ifndef RT_MIN_WAVES_PER_SIMD
#define RT_MIN_WAVES_PER_SIMD 6
#endif
#ifndef RT_MIN_WAVES_PER_SIMD_MANY
#define RT_MIN_WAVES_PER_SIMD_MANY RT_MIN_WAVES_PER_SIMD /* the > 64-model instantiation (measured at 5 as well: see DESIGN.md §4.12) */
#endif
#ifndef RT_MIN_WAVES_PER_SIMD_FLAT
#define RT_MIN_WAVES_PER_SIMD_FLAT 8
#endif
#define RT_PAIR_BYTES 64            /* sizeof(DPair): one record of the top-of-tree cache (asserted in rt_records.h) */
#define RT_STAGED_PIXEL_BYTES 16    /* a staged colour: one float4 per pixel and frame (KArgs::staging) */
#define RT_LDS_BYTES_PER_CU (160 * 1024)
#define RT_MAX_FILTER_EXT_WORDS 32  /* models beyond 63 are tracked in up to 32 extension words of the candidate mask */
#define RT_TRACE_VARIANTS 12        /* kernel instantiations of the trace kernel (launch_shape: variant) */

/* Frames per fused launch: a budget, not a constant.  A launch ends with a tail as long as one pixel chain, so short
 * frames want many per launch (a rank that renders 1/8 of config 2: 0.108 ms per frame, 7.9 work items per resident wave at 16 frames);
 * long frames must not turn into launches that last seconds.  RT_FUSE_MIN frames always; more — up to RT_FUSE_MAX — while the launch
 * stays under RT_FUSE_TARGET_MS at the frame time MEASURED on the previous fused launches (stop event to stop event — or, for a launch
 * without a predecessor, its own start to stop — polled, never waited for).  BVH scenes (>= 1.3 ms per frame) stay at 16.  RT_FUSE_CAP=n
 * pins it. */
#define RT_FUSE_MIN 16
#define RT_FUSE_MAX 64
#define RT_FUSE_TARGET_MS 20.0
#define RT_FUSE_SLAB_BYTES ((size_t)1536 << 20) /* a staging slab: 16 bytes per pixel and frame; 1920x1080: 48 frames, 3840x2160: 16 (2.1 GB), an eighth of 1080p: 64 */

namespace rt_plan {

/* ---- models [0, nFiltered) go through the conservative filter; beyond 64 models the candidate mask has extWords LDS words (KArgs) */
struct Filtering { int nFiltered = 0, extWords = 0; };
inline Filtering filtering(int nModels)
{
    Filtering f;
    f.nFiltered = nModels;
    if (nModels <= 64) return f;
    const int maxModels = 63 + 32 * RT_MAX_FILTER_EXT_WORDS;
    f.nFiltered = nModels < maxModels ? nModels : maxModels;
    f.extWords = (f.nFiltered - 63 + 31) / 32;
    return f;
}

/* the model a lane of the > 64-model kernels visits after model m once its filtered candidates are used up (m = -1: none visited yet):
 * the first model behind the filtered range, then every further one in index order; a result >= nModels says the lane is done.  The
 * vote and phase A of traverse (rt_kernels.h) share it; tests/many_tail_driver.cpp replays it on the host. */
RT_HD int next_unfiltered_model(int m, int nFiltered) { return m < nFiltered - 1 ? nFiltered : m + 1; }

/* a wave's LDS region: traversal stack + pixel fields + (more than 64 models) the mask extension: summary + words + the MANY variant's bounce row */
inline size_t wave_lds_bytes(int stackEntries, int extWords)
{
    return (size_t)(stackEntries + RT_PIXEL_FIELDS + (extWords ? 2 + extWords : 0)) * RT_WAVE * sizeof(uint32_t);
}

/* ---- the BVH trace kernels' workgroups (round 6).  A CU keeps 4 x RT_MIN_WAVES_PER_SIMD waves of them (VGPR bound) if the LDS allows:
 * a wave needs (stack + pixel fields + mask extension) x 256 B.  What the CU's 160 KB leave over becomes the top-of-tree cache — one copy
 * per WORKGROUP, so the fewer, larger workgroups the more records it holds: 12 waves (2 groups per CU) unless RT_WAVES_PER_GROUP says
 * otherwise.  Pure arithmetic on the scene's tree height and model count (no device query): every context, the multi-device upload and
 * rt_debug_layout agree on it.  choose_variant confirms the occupancy with the runtime's own query.
 * wantWaves = RT_WAVES_PER_GROUP (default RT_MAX_WAVES_PER_GROUP); hotKBSet / hotKB = RT_HOT_KB, a cap on the cache. */
struct GroupPlan { int wavesPerGroup = 1; int cacheRecords = 0; };
inline GroupPlan plan_groups(int maxHeight, int nModels, int wantWaves, bool hotKBSet, long long hotKB)
{
    GroupPlan g;
    const size_t waveBytes = wave_lds_bytes(maxHeight, filtering(nModels).extWords);
    int wavesPerCU = 4 * RT_MIN_WAVES_PER_SIMD;
    if ((size_t)wavesPerCU * waveBytes > RT_LDS_BYTES_PER_CU) wavesPerCU = (int)(RT_LDS_BYTES_PER_CU / waveBytes);
    if (wavesPerCU < 1) return g;
    int want = wantWaves;
    if (want < 1) want = 1;
    if (want > RT_MAX_WAVES_PER_GROUP) want = RT_MAX_WAVES_PER_GROUP;
    while (want > 1 && wavesPerCU % want) want--; /* whole groups fill the CU's wave slots */
    const int groupsPerCU = wavesPerCU / want;
    /* LDS is handed out in blocks: keep 1 KB per group clear of the nominal share */
    const long long share = (long long)RT_LDS_BYTES_PER_CU / groupsPerCU - 1024 - (long long)want * (long long)waveBytes;
    long long records = share > 0 ? share / RT_PAIR_BYTES : 0;
    if (hotKBSet) { const long long cap = hotKB * 1024 / RT_PAIR_BYTES; if (cap < records) records = cap < 0 ? 0 : cap; }
    if (records > (1 << 16)) records = 1 << 16;
    if (records < 16) return g; /* not worth a workgroup: single-wave groups, no cache */
    g.wavesPerGroup = want;
    g.cacheRecords = (int)records;
    return g;
}

/* ---- which kernel instantiation, workgroup shape and LDS a launch gets */
/* the > 64-model (chunked) BVH instantiation: also of the passes that launch_shape does not size (rt_context.hip, the AOV pass) */
inline bool many_models(int nChunks, bool flat) { return nChunks > 0 && !flat; }

struct SceneShape {
    bool flat = false;            /* every model root is a leaf: the FLAT variant */
    bool stats = false;
    int stackEntries = 0, extWords = 0, nChunks = 0;
    uint32_t hotUnits = 0;        /* BVH: units of the top-of-tree cache, 0 = none ... */
    int wavesPerGroup = 1;        /* ... and the waves that share it (plan_groups) */
    int poolCells = 0;            /* FLAT: the chain pool's cells, 0 = no pool (RT_POOL=0) ... */
    int poolWaves = 1;            /* ... the waves that share it (RT_POOL_WAVES) ... */
    int poolMinItems = 4;         /* ... and the (tile, frame) items per resident wave a launch needs to use it (RT_POOL_MIN_ITEMS) */
    int numCUs = 256;
};
struct LaunchShape {
    bool pooled = false;          /* FLAT, as multi-wave workgroups around the chain pool */
    bool many = false;            /* the > 64-model (chunked) BVH instantiation */
    bool hot = false;             /* multi-wave workgroups: the BVH top-of-tree cache, or the FLAT chain pool */
    uint32_t hotUnits = 0;        /* the shared LDS region in front of the waves' regions, in 16-byte units */
    int wavesPerGroup = 1, blockThreads = RT_WAVE;
    int poolCells = 0;
    int waveLdsDwords = 0;
    size_t ldsBytes = 0;
    int variant = 0;              /* kernel instantiation = slot of the occupancy cache: stats + 2 flat + 4 many + 6 hot, < RT_TRACE_VARIANTS */
};
inline LaunchShape launch_shape(const SceneShape& s, long long tiles, int nFrames)
{
    LaunchShape l;
    const size_t coldBytes = s.flat ? (size_t)2 * RT_WAVE * 16 : 0; /* the FLAT variant keeps its pixel records in LDS (rt_kernels.h, PX_COLD) */
    const size_t waveBytes = wave_lds_bytes(s.stackEntries, s.extWords) + coldBytes;
    /* pooled for launches with enough work only: a pooled workgroup is 16 persistent waves that leave together, and a launch with a few items
     * per wave is all tail (config 1, 256 x 256: + 11 % with the pool) — at least poolMinItems (tile, frame) pairs per wave the chip keeps resident */
    l.pooled = s.flat && s.poolCells > 0 &&
               tiles * (nFrames > 0 ? nFrames : 1) >= (long long)s.poolMinItems * s.numCUs * 4 * RT_MIN_WAVES_PER_SIMD_FLAT;
    l.hotUnits = s.flat ? (l.pooled ? (uint32_t)(RT_POOL_DWORDS / 4u) : 0u) : s.hotUnits;
    l.wavesPerGroup = s.flat ? (l.pooled ? s.poolWaves : 1) : (l.hotUnits ? s.wavesPerGroup : 1);
    l.blockThreads = RT_WAVE * l.wavesPerGroup;
    l.ldsBytes = (size_t)l.hotUnits * 16 + (size_t)l.wavesPerGroup * waveBytes;
    l.poolCells = l.pooled ? s.poolCells : 0;
    l.waveLdsDwords = (int)(waveBytes / sizeof(uint32_t));
    l.many = many_models(s.nChunks, s.flat);
    l.hot = l.hotUnits > 0;
    l.variant = (s.flat ? 2 : l.many ? 4 : 0) + (s.stats ? 1 : 0) + (l.hot ? 6 : 0);
    return l;
}

/* ---- pixel records (KArgs::pxCold) of one launch slot: every wave the grid can have, + one workgroup of slack */
inline long long record_waves(long long residentGroups, int wavesPerGroup, int gridOverride)
{
    const long long resWaves = residentGroups * wavesPerGroup;
    return (gridOverride > resWaves ? gridOverride : resWaves) + wavesPerGroup;
}

/* ---- the work of one trace kernel: part `part` of `parts` of a launch.
 * Queue position q of part p is entry q*parts + p of the (longest chain first) tile order, so the parts are disjoint and equally heavy.
 * Each kernel is given as many workgroups as the chip keeps resident, never more waves than it has work items.  The tile counter of the
 * kernel's stream counts monotonically across launches; the kernel (rt_kernels.h, the persistent loop's first position and its queue
 * fetch) works it like this:
 *   - a wave with index gw < launchItems, when queueStart = 0, takes position gw directly (the first `byIndex` positions);
 *   - every other position is one atomicAdd on the counter: position = old value - tileQueueBase;
 *   - a fetch that returns a position >= launchItems ends the wave's fetching: every wave of the grid overshoots exactly once.
 * So the counter advances by (items - byIndex) + gridWaves, and the next launch's positions start where this one's end (queueNext).  If
 * the host's count drifts by one, tiles go unrendered in every later launch on that stream. */
struct Work {
    int tiles = 0, nFrames = 1;
    bool flat = false;
    int spp = 1;                  /* RtParams::numRaysPerPixel */
    int frameGroupOverride = 0;   /* RT_FRAME_GROUP (0 = the rule below) */
    int gridOverride = 0;         /* RT_GRID: waves of the grid (0 = resident) */
    long long residentGroups = 0; /* workgroups the chip keeps resident (occupancy query x CUs) */
    int wavesPerGroup = 1;
};
struct PartPlan {
    int partTiles = 0;
    int frameGroup = 1, frameGroupShift = 0, frameGroups = 1;
    long long items = 0;          /* queue positions: (tile, frame group) pairs */
    int grid = 0;                 /* workgroups */
    unsigned long long gridWaves = 0, byIndex = 0;
    int queueStart = 0;           /* 1: every position, a wave's first included, comes from the queue */
    unsigned long long tileQueueBase = 0, queueNext = 0; /* this launch's queue base; the counter after it */
};
inline PartPlan plan_part(const Work& w, int part, int parts, unsigned long long queueNext)
{
    PartPlan pp;
    const bool staged = w.nFrames > 1;
    pp.partTiles = (w.tiles - part + parts - 1) / parts;
    /* frames per item: 1 = the most items and the shortest tail.  The FLAT scenes' per-frame chains are short and uniform; there one
     * pixel set-up per group of frames is worth 7 % (config 2: 0.765 -> 0.710 ms/frame at groups of 4) as long as every resident wave
     * still gets >= 8 items; fewer items than that, or groups of 8+, lose it to the tail again, and the BVH scenes gain nothing
     * measurable (profiles/r02_frame_group_sweep.txt; their kernel variants are compiled without groups). */
    int group = 1;
    if (staged && w.flat && w.spp < 65536) {
        if (w.frameGroupOverride > 0) group = w.frameGroupOverride;
        else
            while (group < 4 && 2 * group <= w.nFrames &&
                   (long long)pp.partTiles * ((w.nFrames + 2 * group - 1) / (2 * group)) >= 8 * w.residentGroups * w.wavesPerGroup)
                group *= 2;
        if (group > w.nFrames) group = w.nFrames;
    }
    pp.frameGroup = group;
    while ((2 << pp.frameGroupShift) <= group) pp.frameGroupShift++;
    pp.frameGroups = staged ? (w.nFrames + group - 1) / group : 1;
    pp.items = (long long)pp.partTiles * pp.frameGroups;
    /* the grid: workgroups of wavesPerGroup persistent waves each — as many as the chip keeps resident, never more waves than there
     * are items (rounded up to whole workgroups: a wave without an item of its own goes to the queue, finds it empty and ends) */
    const int wpb = w.wavesPerGroup;
    long long wantWaves = w.residentGroups * wpb < pp.items ? w.residentGroups * wpb : pp.items;
    if (w.gridOverride > 0) wantWaves = w.gridOverride < pp.items ? w.gridOverride : pp.items;
    pp.grid = (int)((wantWaves + wpb - 1) / wpb);
    pp.gridWaves = (unsigned long long)pp.grid * wpb;
    pp.byIndex = pp.gridWaves < (unsigned long long)pp.items ? pp.gridWaves : (unsigned long long)pp.items;
    /* One kernel alone: all its workgroups become resident at once, the first `grid` positions go by blockIdx and only the rest
     * through the queue.  Two kernels sharing the chip: workgroups are dispatched as slots free up, possibly late, so every
     * position — the longest chains first — comes from the queue. */
    pp.queueStart = parts == 2 ? 1 : 0;
    const unsigned long long direct = pp.queueStart ? 0ull : pp.byIndex;
    pp.tileQueueBase = queueNext - direct;
    pp.queueNext = queueNext + (unsigned long long)pp.items - direct + pp.gridWaves;
    return pp;
}

/* ---- the staging slabs of fused launches and the frames per fused launch */
inline size_t frames_in(size_t slabBytes, size_t nPix) { return slabBytes / (nPix * RT_STAGED_PIXEL_BYTES); }

/* frames a slab is made for: as many as fit the budget (RT_FUSE_SLAB_BYTES, or RT_FUSE_SLAB_MB), between RT_FUSE_MIN and RT_FUSE_MAX, and
 * at least this launch's */
inline size_t slab_frames(size_t nPix, size_t budgetBytes, int nFrames)
{
    size_t f = nPix ? frames_in(budgetBytes, nPix) : RT_FUSE_MAX;
    f = f < RT_FUSE_MIN ? RT_FUSE_MIN : f > RT_FUSE_MAX ? RT_FUSE_MAX : f;
    return f < (size_t)nFrames ? (size_t)nFrames : f;
}

/* RT_FUSE_CAP=v: the cap pinned to v (at most RT_FUSE_MAX); 0 = not pinned */
inline int pinned_fuse_cap(int v) { return v >= 1 ? (v > RT_FUSE_MAX ? RT_FUSE_MAX : v) : 0; }

/* the cap from one measured fused launch (ms over its frames): as many frames as fit RT_FUSE_TARGET_MS, between RT_FUSE_MIN and
 * RT_FUSE_MAX, never more than the smaller of the slabs made so far holds (they are sized once: slab_frames), but never below RT_FUSE_MIN */
struct FuseCap { double msPerFrame = 0; int cap = RT_FUSE_MIN; };
inline FuseCap fuse_cap(float ms, int frames, size_t nPix, const size_t slabBytes[2])
{
    FuseCap f;
    f.msPerFrame = (double)ms / frames;
    int cap = (int)std::ceil(RT_FUSE_TARGET_MS / f.msPerFrame);
    cap = cap < RT_FUSE_MIN ? RT_FUSE_MIN : cap > RT_FUSE_MAX ? RT_FUSE_MAX : cap;
    size_t slab = 0;
    for (int b = 0; b < 2; b++)
        if (slabBytes[b] && (slab == 0 || slabBytes[b] < slab)) slab = slabBytes[b];
    if (nPix && slab) {
        const size_t holds = frames_in(slab, nPix);
        if ((size_t)cap > holds) cap = holds < RT_FUSE_MIN ? RT_FUSE_MIN : (int)holds;
    }
    f.cap = cap;
    return f;
}

/* ---- the launch tuner (RtContext::Tuner): suspension threshold 3/8 or 4/8.  A launch is timed for it on BVH scenes only (the FLAT kernel
 * does not suspend), when staged, of >= 8 frames, without stats, once >= 48 frames have been rendered at this size (short runs keep 3/8) */
inline bool tuner_samples(bool flat, bool staged, int nFrames, bool stats, long long framesSinceResize)
{
    return !flat && staged && nFrames >= 8 && !stats && framesSinceResize >= 48;
}
/* after 3 samples each (ms[c] / n[c]: summed ms per frame of candidate c = 3/8, 4/8): 4 only when it is more than 1 % faster; 0 = not yet */
inline int tuner_decision(const double ms[2], const int n[2])
{
    if (n[0] < 3 || n[1] < 3) return 0;
    return (ms[1] / n[1] < 0.99 * (ms[0] / n[0])) ? 4 : 3; /* 4/8 has to win by more than the noise */
}

} // namespace rt_plan
