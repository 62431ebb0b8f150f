/*
 * rt_denoise.h — an edge-avoiding a-trous filter guided by the first-hit buffers of rt_aov.h (exported by libraytrace_hip.so,
 * plain C).
 *
 * A progressive path tracer shows noise for its first hundreds of frames.  rt_aov.h yields what a denoiser steers by — per
 * pixel the object, the world normal, the world position and the base colour of what the camera ray hit first; this header is
 * the denoiser: a 5 x 5 B3-spline stencil applied `iterations` times with its taps 1, 2, 4, ... pixels apart (Dammertz et al.,
 * "Edge-Avoiding A-Trous Wavelet Transform for fast Global Illumination Filtering", HPG 2010), every tap weighted down by how
 * far its normal, its position and its colour are from the centre's, and never taken across an object's outline.
 *
 * Kept apart from rt_abi.h, whose text is pinned: this header includes rt_aov.h and adds one type and four calls.
 *
 * ---- The arithmetic (a contract, like everything this library computes: every output bit is defined) -----------------------
 * IEEE binary32, one rounding per operation written below, no contraction; rt_exp and rt_div are include/rt_math.h's; dot(a, b)
 * is a.x*b.x + a.y*b.y + a.z*b.z summed left to right.  "Finite" means: the exponent field is not all ones.  Per pixel p, with
 * in = d_rgba_in[p] and a = d_aov[p] (csrc/rt_denoise_math.h is this text as code, shared by the kernels and a host test):
 *
 * Host, once per call:  aN = 1 / (sigmaNormal * sigmaNormal), aP = 1 / (sigmaPlane * sigmaPlane), aC = 1 / (sigmaColour *
 *   sigmaColour)  (a product, then an IEEE divide);  aC_i = aC * 4^i for pass i (4^i is exact).
 *
 * Prepare:  c[k] = in[k] * scale (k = 0, 1, 2), alpha = in[3] (never touched again).  mask = 0.  If demodulate != 0, a.object >= 0,
 *   (a.hit & 3) == RT_AOV_HIT_OPAQUE and c[0..2] are finite: for every k with a.albedo[k] > 1/256:  c[k] = rt_div(c[k], a.albedo[k])
 *   and bit k of mask is set.  Every other channel and pixel is neither divided here nor multiplied back at the end.
 *   The guide of p is n = a.normal, pos = a.pos, object = a.object.
 *
 * iterations == 0:  out = (c[0], c[1], c[2], alpha), computed with mask = 0 whatever demodulate says.
 *
 * Pass i = 0 ... iterations - 1, spacing s = 2^i, from the colours c of the pass before (pass 0: of Prepare) to new colours c':
 *   p is NOT filtered in this pass, c'(p) = c(p), when a.object < 0 (a miss) or a component of c(p) is not finite — so a miss and a
 *   pixel whose input is NaN or infinite come out as their scaled input.  Otherwise
 *     sum_w = sum_c[0..2] = +0;  for dy = -2 ... 2 (outer), dx = -2 ... 2 (inner), q = p + (dx * s, dy * s):
 *       the tap is skipped when q is outside the image, when object(q) != object(p), or when a component of c(q) is not finite;
 *       dn = n(p) - n(q);  d = pos(q) - pos(p);  t = dot(n(p), d);  dc = c(p) - c(q)          (componentwise, c's three channels)
 *       e  = (dot(dn, dn) * aN + (t * t) * aP) + dot(dc, dc) * aC_i
 *       w  = (h[dy + 2] * h[dx + 2]) * rt_exp(-e),   h = (1/16, 1/4, 3/8, 1/4, 1/16)   (the product of two h is exact)
 *       sum_w += w;  sum_c[k] += w * c(q)[k]
 *     c'(p)[k] = rt_div(sum_c[k], sum_w).
 *   The centre tap (dy = dx = 0) is a tap like the others: e = 0, w = 9/64, so sum_w > 0 whenever the guide of p is finite
 *   (parameters whose aN, aP or aC_i is not finite are refused, so 0 * a is 0).  The guide is taken as it is: a hit pixel whose normal
 *   or position holds a NaN or an infinity gets e = NaN in its own centre tap and comes out NaN in its three colour channels, and is
 *   then skipped as a tap by its neighbours in the passes that follow.
 *   (A skipped tap adds nothing.  The code adds +0 instead: no sum can be -0 — each starts at +0 and x + (-x) = +0 — so x + 0 = x,
 *   bit for bit.)
 *
 * Finish (fused into the last pass):  out[k] = bit k of mask ? c'[k] * a.albedo[k] : c'[k];  out[3] = alpha.
 *
 * The source image is never written.  Rows: row 0 at the bottom, as everywhere in this library (the filter itself is symmetric).
 */
#ifndef RT_DENOISE_H
#define RT_DENOISE_H

#include "rt_aov.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_DENOISE_MAX_ITERATIONS 8

typedef struct RtDenoiseParams {   /* 32 bytes */
    uint32_t struct_size;          /* = sizeof(RtDenoiseParams): handshake, RT_ERR_ABI_MISMATCH otherwise */
    int32_t  iterations;           /* 0..8 passes; pass i uses tap spacing 2^i pixels; 0 = copy */
    float    sigmaColour;          /* > 0; halves with every pass */
    float    sigmaNormal;          /* > 0 */
    float    sigmaPlane;           /* > 0; world units, distance of the tap's hit point from the centre's tangent plane */
    int32_t  demodulate;           /* != 0: filter colour / albedo on opaque first hits, multiply back afterwards */
    float    scale;                /* the input colour is multiplied by this first (1 / frames for an accumulated sum) */
    int32_t  reserved;             /* must be 0 */
} RtDenoiseParams;

/* Fills *out with valid parameters (struct_size set; 5 iterations, demodulation on, scale 1).  RT_ERR_INVALID_ARG for null. */
int rt_denoise_default_params(RtDenoiseParams* out);

/* The filter alone, on caller-owned device memory of the context's device: d_rgba_in width x height RGBA32F, d_aov width x height
 * RtPixelAov, d_rgba_out width x height RGBA32F; each 16-byte aligned, row 0 at the bottom; d_rgba_out overlaps neither input.
 * Only enqueues: it runs on the stream the context renders on (rt_set_stream is respected), behind everything already requested, and
 * is complete after rt_synchronize.  Needs no scene and no rt_resize: width and height are the call's own.
 *
 * This is also the call for an image rendered by several GPUs: gather the image (rt_gather_accumulated_to_device) and the AOV
 * records of all the parts into device memory of one GPU, then filter there.  A context that owns only part of the image cannot
 * filter — a pass with spacing 16 needs rows its strips do not have — so all three filter calls return RT_ERR_STATE on a context
 * with rt_set_partition(..., part_count > 1). */
int rt_denoise_buffers(RtContext* ctx, const RtDenoiseParams* p, int width, int height,
                       const void* d_rgba_in, const void* d_aov, void* d_rgba_out);

/* Convenience for a context that owns the whole image.  Source: the context's AccumulatedRender (use_accumulated != 0) or FrameRender,
 * as it stands — AccumulatedRender is a sum, so the caller puts 1 / frames into p->scale.  Guide: the AOV pass of frame `aov_frame`
 * (>= 1), exactly as rt_render_aov_to_device produces it, into scratch the library owns.  bytes = rows * W * 16.
 *
 * rt_denoise writes host memory and is synchronous.  rt_denoise_to_device writes device memory of the context's device (validated like
 * rt_render_aov_to_device's pointer; it must not overlap the source image) and only enqueues, like rt_denoise_buffers.
 *
 * All three calls change nothing a caller can see: render targets, accumulation, frame counter, RtCounters and the context's watchdog
 * word are as before.  Frames rt_render_frame holds back are launched first.  Scratch (two colour images, the packed guide image, the
 * AOV records) lives in the context, grows on demand and is freed by rt_destroy.
 *
 * Errors: RT_ERR_INVALID_ARG for a null context or pointer, iterations outside 0..8, a sigma that is <= 0 or not finite, a sigma so
 * small that 1 / sigma^2 (times 4^(iterations - 1) for the colour) is not finite, a scale that is not finite, reserved != 0,
 * aov_frame < 1, a wrong `bytes`, width or height < 1, and misaligned, overlapping or wrong-device
 * memory; RT_ERR_ABI_MISMATCH for a wrong struct_size; RT_ERR_STATE before rt_resize, rt_upload_scene or rt_set_params (the two
 * context calls) and on a partitioned context (all three); RT_ERR_HIP when the traversal watchdog fired in the internal AOV pass,
 * reported as rt_render_aov (rt_denoise: when it returns) and rt_render_aov_to_device (rt_denoise_to_device: by the next
 * rt_synchronize, once) report theirs.  rt_denoise also fails, like every call that hands the context's pixels to the host, when the
 * context's own watchdog word is set. */
int rt_denoise(RtContext* ctx, const RtDenoiseParams* p, int use_accumulated, int aov_frame, float* rgba, size_t bytes);
int rt_denoise_to_device(RtContext* ctx, const RtDenoiseParams* p, int use_accumulated, int aov_frame, void* d_rgba, size_t bytes);

#ifdef __cplusplus
} /* extern "C" */

static_assert(sizeof(RtDenoiseParams) == 32, "RtDenoiseParams must be 32 bytes");
#endif

#endif /* RT_DENOISE_H */
