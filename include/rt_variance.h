/*
 * rt_variance.h — per-pixel luminance moments of a progressive render and an a-trous filter steered by the variance they give
 * (exported by libraytrace_hip.so, plain C).
 *
 * rt_denoise.h stops at colour edges with one global sigmaColour that halves from pass to pass: it filters a pixel that has
 * converged over 256 carried frames as hard as one that lost its history a frame ago, and after rt_reproject_accumulated every image
 * holds both kinds of pixel.  The remedy is a per-pixel estimate of the variance of the mean (Schied et al., "Spatiotemporal
 * Variance-Guided Filtering", HPG 2017): accumulated over time, carried across camera and object moves with the colour, scaling the
 * filter's luminance edge-stop — so the filter gets out of the way where the image has converged — and itself filtered from pass to
 * pass.  No trace kernel knows about this header: AccumulatedRender is a sum whose alpha is the per-pixel frame count, and that is
 * all the estimate needs.
 *
 * The pipeline of a moving camera, with the two new steps marked *:  rt_set_params (the new camera), rt_reproject_accumulated[_moving]
 * (..., d_cur_aov_out), * rt_variance_carry (the same parameters, the same records), rt_render_frames, * rt_variance_update,
 * rt_denoise_variance_to_device.  No step copies through the host.
 *
 * Kept apart from rt_abi.h, whose text is pinned: this header includes rt_reproject.h and rt_denoise.h and adds one type and ten calls.
 *
 * ---- The arithmetic (a contract, like everything this library computes: every output bit is defined) -----------------------
 * IEEE binary32, one rounding per operation written below, no contraction; rt_div, rt_exp, rt_sqrt, rt_max and rt_abs are
 * include/rt_math.h's; dot(a, b) is a.x*b.x + a.y*b.y + a.z*b.z summed left to right;  lum(c) = (0.2126f * c[0] + 0.7152f * c[1]) +
 * 0.0722f * c[2].  "Finite" means: the exponent field is not all ones.  (csrc/rt_variance_math.h is this text as code, shared by the
 * kernels and a host test.)
 *
 * The moments image.  W x H RGBA32F, row 0 at the bottom; pixel p holds M = (sum of L, sum of L * L, +0, nb): L is the luminance of one
 * BATCH MEAN — the mean of the frames that were added to the sum between two updates — and nb the number of batches.  It is a "sum
 * with its count in alpha", and channel 2 is +0 by construction, so rt_reproject_buffers and rt_reproject_buffers_moving carry it
 * with the arithmetic they have: the blended means of L and L * L times the blended, capped count, and rt_div(+0, nb) = +0, w * +0 =
 * +0, +0 * n = +0 keep channel 2 at +0.  No reprojection kernel of its own exists.  Batches are differences of the sum, not
 * FrameRender: a fused rt_render_frames(17) is simply one batch.  The estimate is the variance of batch means, hence exact for equal
 * batches and an approximation otherwise; and the snapshot the differences are taken against must be REBASED whenever the sum is
 * replaced rather than added to — after rt_reset_accumulation, rt_write_accumulated and any reprojection (the context calls below:
 * rt_variance_reset, rt_variance_carry).
 *
 * Update, per pixel:  now = d_sum[p], snap = d_snapshot[p], M = d_moments[p].
 *   rebase != 0:  snap := now, nothing else.
 *   Otherwise  dn = now.a - snap.a.  When dn > 0 and all eight values of now and snap are finite:  b[k] = rt_div(now[k] - snap[k], dn)
 *   (k = 0, 1, 2);  L = lum(b);  Q = L * L;  and when Q is finite  M := (M.x + L, M.y + Q, +0, M.w + 1).  In every other case M is left as
 *   it is.  Then snap := now.
 *   (The test of Q is not in the first design of this pass.  Finite sums can have a difference, a luminance or a square that
 *   overflows; one such batch would leave M non-finite — "variance unknown" — until the next reset, however many good batches follow.
 *   Dropping the batch costs one sample.  A finite Q implies a finite L.)
 *
 * Prepare, per pixel:  in = d_rgba_in[p], a = d_aov[p], M = d_moments[p].
 *   raw[k] = in[k] * scale;  c and the demodulation mask from raw exactly as Prepare of rt_denoise.h has them;  the guide likewise.
 *   1. When M.w >= 2 (a NaN fails this) and M.x, M.y, M.w are finite:  mu = rt_div(M.x, M.w);  d = rt_max(M.y - mu * M.x, +0)  (the
 *      difference of two nearly equal sums may cancel below zero);  var = rt_div(d, M.w * (M.w - 1)).
 *   2. Otherwise var = unknownVariance.  (After a reprojection nb is a blend: 1.5 batches are fewer than two.)
 *   3. Into the units of the filtered colour: when mask != 0 and l_in = lum(raw) is finite and > 0:  k = rt_div(lum(c), l_in);
 *      var = var * (k * k).  Otherwise var is unchanged.
 *   4. If var is then not finite, var = unknownVariance.
 *   So var is finite and >= 0.  The pixel travels as (c[0], c[1], c[2], var): alpha no longer rides in the colour quantity.
 *   `scale` normalises, it is not an exposure: in * scale must be in the units of the batch means — scale = 1 for a resolved image,
 *   1 / frames for a sum with one global count — because var is not multiplied by scale * scale.  (The first design left that open;
 *   a caller's exposure belongs behind the filter.)
 *
 * iterations == 0:  out = (raw[0], raw[1], raw[2], in[3]); neither the moments nor the records are read.
 *
 * Pass i = 0 ... iterations - 1, spacing s = 2^i, from (c, var) of the pass before to (c', var').  l(x) = lum(c(x)).
 *   p is NOT filtered, c'(p) = c(p) and var'(p) = var(p), when a.object < 0 or a component of c(p) is not finite.  Otherwise, with
 *   "q is used" meaning: q is inside the image, object(q) == object(p) and c(q)[0..2] are finite (the rule of rt_denoise.h):
 *     Prefilter.  sum_k = sum_g = +0;  for dy = -1, 0, 1 (outer), dx = -1, 0, 1 (inner), q = p + (dx * s, dy * s) used:
 *       k = hg[dy + 1] * hg[dx + 1], hg = (1/4, 1/2, 1/4);  sum_k += k;  sum_g += k * var(q).      g = rt_div(sum_g, sum_k).
 *       The 3 x 3 Gaussian is taken on the pass's own lattice, not on adjacent pixels: every tap stays inside the one-sub-lattice tile
 *       rt_dn_pass_kernel's staging holds (two-record halo, 20,736 B of LDS at every spacing).  The centre is always used: sum_k >= 1/4.
 *     invL = rt_div(1, sigmaLuminance * rt_sqrt(g) + 0x1p-13f).     sigmaLuminance is the same in every pass: the variance shrinks.
 *     sum_w = sum_c[0..2] = sum_v = +0;  for dy = -2 ... 2 (outer), dx = -2 ... 2 (inner), q = p + (dx * s, dy * s) used:
 *       dn, d, t as in rt_denoise.h;  e = (dot(dn, dn) * aN + (t * t) * aP) + rt_abs(l(p) - l(q)) * invL
 *       w = (h[dy + 2] * h[dx + 2]) * rt_exp(-e);  sum_w += w;  sum_c[k] += w * c(q)[k];  sum_v += (w * w) * var(q)
 *     c'(p)[k] = rt_div(sum_c[k], sum_w);  var'(p) = rt_div(sum_v, sum_w * sum_w).
 *   The centre tap has e = 0 and w = 9/64 as in rt_denoise.h (invL <= 2^13 is finite, so 0 * invL = 0).  Since the w are >= 0, the sum
 *   of w * w is at most sum_w * sum_w: var' never exceeds the largest var of its taps by more than rounding, so it stays finite and
 *   0 * infinity cannot arise for any var below 2^120 — a luminance error of 2^60.  A hit pixel with a NaN guide comes out NaN in colour
 *   AND var and is then skipped, with its var, by its neighbours' taps and prefilters.
 *
 * Finish (fused into the last pass):  out[k] = bit k of mask ? c'[k] * a.albedo[k] : c'[k];  out[3] = in[3], fetched from d_rgba_in
 * where the last pass writes.  No input is ever written.
 */
#ifndef RT_VARIANCE_H
#define RT_VARIANCE_H

#include "rt_reproject.h"
#include "rt_denoise.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct RtVarianceDenoiseParams {   /* 40 bytes */
    uint32_t struct_size;          /* = sizeof(RtVarianceDenoiseParams): handshake, RT_ERR_ABI_MISMATCH otherwise */
    int32_t  iterations;           /* 0..RT_DENOISE_MAX_ITERATIONS passes; pass i uses tap spacing 2^i pixels; 0 = scaled copy */
    float    sigmaLuminance;       /* > 0; in standard deviations of the mean; the same in every pass */
    float    sigmaNormal;          /* > 0 */
    float    sigmaPlane;           /* > 0; world units */
    int32_t  demodulate;           /* != 0: filter colour / albedo on opaque first hits, multiply back afterwards */
    float    scale;                /* the input colour is multiplied by this first; see Prepare: a normalisation, not an exposure */
    float    unknownVariance;      /* >= 0, finite: the variance of a pixel with fewer than two batches */
    int32_t  reserved[2];          /* must be 0 */
} RtVarianceDenoiseParams;

/* Fills *out with valid parameters (struct_size set; 5 iterations, demodulation on, scale 1).  RT_ERR_INVALID_ARG for null. */
int rt_denoise_variance_default_params(RtVarianceDenoiseParams* out);

/* "Update" above, on caller-owned device memory of the context's device: three width x height RGBA32F images, 16-byte aligned, no two
 * of them overlapping.  d_sum is never written; rebase != 0 writes d_snapshot alone.  Only enqueues, on the stream the context renders
 * on (rt_set_stream is respected), behind everything already requested.  Needs no scene and no rt_resize, and — every pixel is its
 * own — works on a context that owns part of an image. */
int rt_moments_update_buffers(RtContext* ctx, int width, int height, const void* d_sum, void* d_snapshot, void* d_moments, int rebase);

/* The filter alone, on caller-owned device memory of the context's device: d_rgba_in and d_moments width x height RGBA32F, d_aov
 * width x height RtPixelAov, d_rgba_out width x height RGBA32F; each 16-byte aligned; d_rgba_out overlaps no input.  Only enqueues,
 * like rt_denoise_buffers; needs no scene and no rt_resize; changes nothing of the context.  It needs the whole image: RT_ERR_STATE
 * on a context with rt_set_partition(..., part_count > 1) — gather the sum, the moments and the records first, as for
 * rt_denoise_buffers. */
int rt_denoise_variance_buffers(RtContext* ctx, const RtVarianceDenoiseParams* p, int width, int height,
                                const void* d_rgba_in, const void* d_moments, const void* d_aov, void* d_rgba_out);

/* The context's own moments image and snapshot, for its rows: allocated and zeroed on first use, zeroed again by rt_resize, freed by
 * rt_destroy.  All zero is the state after rt_reset_accumulation: no batch, and a snapshot equal to the empty sum.
 *
 * rt_variance_update: "Update" from AccumulatedRender (the context's own or the bound one) as it stands behind every frame requested
 *   so far; frames rt_render_frame holds back are launched first.  Per pixel, so a context that owns part of the image may call it.
 * rt_variance_reset: moments := 0, snapshot := AccumulatedRender as it stands.  After rt_reset_accumulation or rt_write_accumulated.
 * rt_variance_carry: right after rt_reproject_accumulated[_moving], with the same parameters, the d_prev_aov given to that call and
 *   the records it wrote (its d_cur_aov_out): replaces the moments by their reprojection through rt_reproject_buffers (d_motion ==
 *   NULL; n_objects is then not looked at) or rt_reproject_buffers_moving (otherwise), then rebases the snapshot onto the reprojected
 *   AccumulatedRender.  When that call's AOV pass had its watchdog fire, it left AccumulatedRender as it was; rt_variance_carry then
 *   leaves the moments as they were too — the device decides, by the same word — so sum and moments stay one view's.  (Not in the first
 *   design: moments reprojected by records that are not valid would belong to no image.)
 * These three change the moments and the snapshot and nothing else, and only enqueue.
 *
 * rt_variance_read_moments: the moments into host memory (bytes = rows * W * 16); synchronous; fails, like every call that hands the
 *   context's pixels to the host, when the context's watchdog word is set, and reports (once, RT_ERR_HIP) an unreported watchdog of a
 *   preceding device AOV pass, as rt_resolve does.
 * rt_variance_moments_to_device: the same into device memory that does not overlap the moments; only enqueues.
 * rt_denoise_variance, rt_denoise_variance_to_device: the per-pixel resolve of AccumulatedRender (rt_reproject.h, "Resolve") into
 *   scratch, then the filter above with that image as d_rgba_in — so p->scale applies after the resolve: 1 — the context's moments and
 *   the AOV pass of frame `aov_frame` (>= 1) as rt_denoise runs it.  bytes = rows * W * 16.  Held-back frames, the internal pass's
 *   watchdog and the context's watchdog word are handled exactly as by rt_denoise and rt_denoise_to_device.
 * These four change nothing a caller can see: render targets, frame counter, RtCounters, the watchdog word, moments and snapshot. */
int rt_variance_update(RtContext* ctx);
int rt_variance_reset(RtContext* ctx);
int rt_variance_carry(RtContext* ctx, const RtReprojectParams* p, const void* d_prev_aov, const void* d_cur_aov, const void* d_motion, int n_objects);
int rt_variance_read_moments(RtContext* ctx, float* rgba, size_t bytes);
int rt_variance_moments_to_device(RtContext* ctx, void* d_rgba, size_t bytes);
int rt_denoise_variance(RtContext* ctx, const RtVarianceDenoiseParams* p, int aov_frame, float* rgba, size_t bytes);
int rt_denoise_variance_to_device(RtContext* ctx, const RtVarianceDenoiseParams* p, int aov_frame, void* d_rgba, size_t bytes);

/* Errors: RT_ERR_INVALID_ARG for a null context or pointer (d_motion alone may be null), iterations outside 0..8, a sigma that is <= 0
 * or not finite, a sigmaNormal or sigmaPlane so small that 1 / sigma^2 is not finite, a scale that is not finite, an unknownVariance
 * that is negative or not finite, a reserved word != 0, the parameter errors of rt_reproject.h and rt_motion.h (rt_variance_carry),
 * aov_frame < 1, a wrong `bytes`, width or height < 1 or more than 2^30 pixels, and misaligned, overlapping or wrong-device memory;
 * RT_ERR_ABI_MISMATCH for a wrong struct_size; RT_ERR_STATE before rt_resize (every context call), before rt_upload_scene or
 * rt_set_params (rt_denoise_variance, rt_denoise_variance_to_device), and on a partitioned context (rt_variance_carry and the three
 * filter calls); RT_ERR_HIP for the watchdogs as stated above. */

#ifdef __cplusplus
} /* extern "C" */

static_assert(sizeof(RtVarianceDenoiseParams) == 40, "RtVarianceDenoiseParams must be 40 bytes");
#endif

#endif /* RT_VARIANCE_H */
