/*
 * rt_held_back.h — the frames rt_render_frame holds back, seen from outside (exported by libraytrace_hip.so, plain C).  Test hooks.
 *
 * rt_render_frame holds a frame back while the GPU is still busy with earlier ones: it counts the frame (rt_get_frame) and the held
 * frames leave later as one fused launch, rendered with the state the context has at that moment.  So every entry point that reads what
 * those frames produce, or changes what they depend on, launches them first; tests/flush_table.py lists every entry point with the side
 * of that contract it is on.  Whether a frame is held back is a race between the caller and the GPU.  Two test hooks take the race out:
 *
 *   RT_HOLD_BACK=1 in the environment of rt_create: the context treats the GPU as busy, so every rt_render_frame that may be held back
 *   (coalescing and fusing on, params.accumulate, the context's own stream) is, until a fused launch's worth has gathered
 *   (rt_debug_fused_frames_cap) or a call that needs the frames arrives.  Nothing else changes; unset, nothing changes at all.
 *
 *   The two calls below report how many frames are held.
 *
 * Kept apart from rt_abi.h, whose text is pinned: this header includes it and adds two calls, and restates one declaration of rt_abi.h
 * to say on which side of the contract it is.
 */
#ifndef RT_HELD_BACK_ABI_H
#define RT_HELD_BACK_ABI_H

#include "rt_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Test hook: frames rt_render_frame has counted (rt_get_frame) but holds back, not launched yet; RT_ERR_INVALID_ARG for a null
 * context.  Launches nothing. */
int rt_debug_pending_frames(const RtContext* ctx);

/* Test hook: the largest rt_debug_pending_frames over the multi-context's contexts; RT_ERR_INVALID_ARG for a null handle.  Launches
 * nothing. */
int rt_debug_multi_pending_frames(const RtMulti* m);

/* (declared in rt_abi.h; restated for the contract)  The i-th context of a multi-context is a lookup: it neither reads nor changes
 * what a frame depends on, and launches nothing — frames its contexts hold back stay held. */
RtContext* rt_multi_context(RtMulti* m, int i);

#ifdef __cplusplus
}
#endif

#endif
