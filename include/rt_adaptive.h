/*
 * rt_adaptive.h — render further frames only where the image is still noisy: the 8 x 8 tiles whose relative standard error of the mean
 * luminance exceeds a threshold are selected from the per-pixel variance of rt_variance.h, and rt_adaptive_render_frames renders frames
 * on the selected tiles alone (exported by libraytrace_hip.so, plain C).
 *
 * Every piece beside the tracer already copes with pixels that hold different numbers of frames: AccumulatedRender keeps the per-pixel
 * frame count in alpha, rt_resolve divides per pixel, rt_variance_update takes its batches from per-pixel count differences, the
 * reprojection blends and caps counts.  The tracer itself always rendered every pixel; after a reprojection that keeps 98 % of the
 * history, repairing the other 2 % cost a whole frame.  The trace kernels are not changed for this: a persistent wave takes its tiles
 * from a list, and each pixel's frame is an independent chain seeded by (pixel index, Frame, seed) — so a launch over a shorter list
 * writes, for the listed tiles, exactly the bits a full frame would write there, and touches nothing else.
 *
 * The loop of a caller:  rt_render_frames (a batch), rt_variance_update, rt_adaptive_select, rt_adaptive_render_frames (the next batch
 * on the active tiles), rt_variance_update, rt_adaptive_select, ... until no tile is active; then rt_resolve (the per-pixel divide).
 *
 * Kept apart from rt_abi.h, whose text is pinned: this header includes rt_variance.h and adds two types and seven calls.
 *
 * ---- Tiles ------------------------------------------------------------------------------------------------------------------------
 * The tracer's own:  tilesX = ceil(W / 8), tilesY = ceil(rows / 8), tiles_total = tilesX * tilesY;  `rows` are the context's local
 * rows (rt_local_rows), for rt_adaptive_select_buffers `height`.  Tile t = ty * tilesX + tx covers local rows 8 ty ... 8 ty + 7 and
 * columns 8 tx ... 8 tx + 7, clipped to the image.
 *
 * ---- The error of a pixel (a contract, like everything this library computes: every output bit is defined) ------------------------
 * IEEE binary32, one rounding per operation written below, no contraction; rt_div, rt_sqrt, rt_max and rt_abs are include/rt_math.h's;
 * "finite" means: the exponent field is not all ones.  (csrc/rt_adaptive_math.h is this text as code, shared by the kernel and a host
 * test.)  S = d_sum[p] is the accumulated pixel (sum of r, g, b; frame count in a), M = d_moments[p] the pixel of the moments image of
 * rt_variance.h (sum of L, sum of L * L, +0, batches).
 *   1. If any of the four values of S is not finite:  err = +0.  (Further frames cannot repair that pixel: it must not keep its tile
 *      alive for ever.)
 *   2. Else if maxFrames > 0 and S.a >= (float)maxFrames:  err = +0.
 *   3. Else if S.a < (float)minFrames:  err = +inf.
 *   4. Else if M.w >= 2 fails (a NaN fails it too) or M.x, M.y or M.w is not finite:  err = +inf.  (The variance is unknown; a blended
 *      count of 1.5 batches is fewer than two.)
 *   5. Otherwise  mu = rt_div(M.x, M.w);  d = rt_max(M.y - mu * M.x, +0);  var = rt_div(d, M.w * (M.w - 1))  (steps 1 and 2 of
 *      rt_variance.h's Prepare, to the letter);  err = rt_div(rt_sqrt(var), rt_abs(mu) + darkFloor);  if err is a NaN (infinity times
 *      the zero that the reciprocal of an infinite denominator is), err = +inf.
 *   So err is +inf, or finite and >= +0; never a NaN, never -0.
 *
 * The error of a tile is the maximum of err over the tile's pixels inside the image — of values that are never NaN, so the order of
 * evaluation does not matter.  A tile is ACTIVE iff tileErr > threshold: the comparison is strict, so with threshold = 0 a tile whose
 * pixels all have err = +0 is not active.
 *
 * The tile list holds the active tiles as uint32, in strictly increasing t: the order is part of the contract.  With it go two
 * counts: tiles_active, the length of the list, and pixels_active, the number of pixels inside the image the listed tiles cover.
 *
 * ---- The frames of a list -----------------------------------------------------------------------------------------------------------
 * rt_adaptive_render_frames(ctx, n) renders frames Frame, Frame + 1, ..., Frame + n - 1 of the tiles of the current list.  For every
 * pixel inside the image of a listed tile, in frame order:  AccumulatedRender.rgb += colour, alpha += 1, FrameRender = (colour, 1) —
 * the additions rt_render_frames performs, in its order, with the colours it computes.  Every other pixel of both targets keeps its
 * bits.  The frame counter advances by n whatever the list holds, an empty list included.  RtCounters.pixelFrames advances by
 * pixels_active * n; segments, and the detailed counters under rt_enable_stats, count the listed pixels' work alone.
 *
 * Not in this header:  rt_multi_* forwarding (call the contexts of rt_multi_context one by one);  dilating the active set by a ring of
 * tiles;  per-pixel rather than per-tile masks.
 */
#ifndef RT_ADAPTIVE_H
#define RT_ADAPTIVE_H

#include "rt_variance.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct RtAdaptiveParams {   /* 32 bytes */
    uint32_t struct_size;          /* = sizeof(RtAdaptiveParams): handshake, RT_ERR_ABI_MISMATCH otherwise */
    float    threshold;            /* finite, >= 0: a tile is active while its relative standard error of the mean luminance exceeds this */
    float    darkFloor;            /* finite, > 0, in luminance units: added to |mean| in the divisor, so that a dark pixel is not held to a relative error */
    int32_t  minFrames;            /* >= 0: a pixel with fewer accumulated frames is always in error */
    int32_t  maxFrames;            /* >= 0: a pixel with at least this many frames is never in error; 0 = no cap */
    int32_t  reserved[3];          /* must be 0 */
} RtAdaptiveParams;

typedef struct RtAdaptiveResult {   /* 16 bytes */
    uint32_t tiles_total;          /* tilesX * tilesY of the context's rows */
    uint32_t tiles_active;         /* the length of the list */
    uint32_t pixels_active;        /* pixels inside the image that the listed tiles cover */
    uint32_t reserved;             /* 0 */
} RtAdaptiveResult;

/* Fills *out with valid parameters: struct_size set, threshold 0.05 (a standard error of 5 % of the mean), darkFloor 0.01, minFrames 8,
 * maxFrames 1024.  A starting point, not the result of a measurement.  RT_ERR_INVALID_ARG for null. */
int rt_adaptive_default_params(RtAdaptiveParams* out);

/* Tile errors, list and counts on caller-owned device memory of the context's device: d_sum and d_moments width x height RGBA32F (never
 * written); d_tile_error tiles_total floats; d_tiles tiles_total uint32, of which entries [0, tiles_active) are written and the rest
 * left as they are; d_counts uint32[4] = {tiles_active, pixels_active, 0, 0}.  Each 16-byte aligned; no output overlaps an input or
 * another output.  Only enqueues, on the stream the context renders on (rt_set_stream is respected), behind everything already
 * requested.  Needs no scene and no rt_resize and changes nothing of the context. */
int rt_adaptive_select_buffers(RtContext* ctx, const RtAdaptiveParams* p, int width, int height, const void* d_sum, const void* d_moments,
                               void* d_tile_error, void* d_tiles, void* d_counts);

/* The same from the context's AccumulatedRender (its own or the bound one) and its moments image, for its rows — a context that owns
 * part of an image selects among its own tiles — into buffers the context owns: its tile errors and its CURRENT LIST.  Frames
 * rt_render_frame holds back are launched first.  Synchronous (it hands two numbers to the host, as rt_get_counters does) and fails,
 * like every call that hands the context's pixels to the host, when the context's watchdog word is set.  It does NOT run
 * rt_variance_update: the caller decides where batches end.  *out may be null. */
int rt_adaptive_select(RtContext* ctx, const RtAdaptiveParams* p, RtAdaptiveResult* out);

/* A list from the host in place of a selected one (a region of interest; tests): n entries, strictly increasing, each < tiles_total;
 * n == 0 is the empty list (tiles may then be null).  The tile errors of an earlier rt_adaptive_select stay readable. */
int rt_adaptive_set_tiles(RtContext* ctx, const uint32_t* tiles, int n);

/* The current list into host memory: *n = its length, and — when tiles is not null — its entries, which need capacity >= *n.
 * Synchronous. */
int rt_adaptive_read_tiles(RtContext* ctx, uint32_t* tiles, int capacity, int* n);

/* The tile errors of the last rt_adaptive_select: bytes = tiles_total * 4.  Synchronous. */
int rt_adaptive_read_tile_error(RtContext* ctx, float* err, size_t bytes);

/* "The frames of a list" above.  Only enqueues, behind the frames rt_render_frame holds back; rt_set_stream and bound render targets
 * are respected; the watchdog is the context's own, as for every render launch.  n == 1 (and every frame when frames are not fused:
 * RT_FUSE_FRAMES=0, or no staging memory) is one launch of the trace kernel rt_render_frames would use, over the list; n > 1 leaves
 * in fused launches of up to rt_debug_fused_frames_cap frames whose colours are added in frame order afterwards.  The bits are the same
 * either way.  The tile order, the launch tuner and the frame-time probes of the normal launches are not touched: a later
 * rt_render_frames behaves as if this call had not happened.
 * rt_resize and rt_set_partition drop the list and the tile errors; rt_reset_accumulation, rt_write_accumulated and a reprojection keep
 * them (the geometry is unchanged; the caller selects again when the image changes). */
int rt_adaptive_render_frames(RtContext* ctx, int n);

/* Errors: RT_ERR_INVALID_ARG for a null context, null parameters, a threshold that is negative or not finite, a darkFloor that is <= 0
 * or not finite, minFrames < 0, maxFrames < 0, a reserved word != 0, width or height < 1 or more than 2^30 pixels, misaligned,
 * overlapping or wrong-device memory, a list that is not strictly increasing or names a tile >= tiles_total, n < 0, a null `tiles` with
 * n > 0, a null `n` or a capacity below the list's length (rt_adaptive_read_tiles), a wrong `bytes` or a null `err`;
 * RT_ERR_ABI_MISMATCH for a wrong struct_size; RT_ERR_STATE before rt_resize (every context call), for rt_adaptive_read_tiles and
 * rt_adaptive_render_frames before a list exists (none does after rt_resize), for rt_adaptive_read_tile_error before an
 * rt_adaptive_select since the last rt_resize, and for rt_adaptive_render_frames before rt_upload_scene or rt_set_params and when
 * params.accumulate == 0 (a frame that adds nothing has nothing to be selective about); RT_ERR_HIP for the watchdog as stated above. */

#ifdef __cplusplus
} /* extern "C" */

static_assert(sizeof(RtAdaptiveParams) == 32, "RtAdaptiveParams must be 32 bytes");
static_assert(sizeof(RtAdaptiveResult) == 16, "RtAdaptiveResult must be 16 bytes");
#endif

#endif /* RT_ADAPTIVE_H */
