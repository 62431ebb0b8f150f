/*
 * rt_primary.h — the per-launch table of ray-origin constants, seen from outside (exported by libraytrace_hip.so, plain C).
 *
 * In a scene without trees rendered without defocus, every camera ray of a launch starts at one point, and the trace kernel reads what
 * depends on that point and the scene alone from a table the host fills once per launch (ray-tracing_amd/csrc/rt_primary.h, DESIGN.md
 * §4.13).  Results never depend on it; RT_PRIMARY=0 in the environment of rt_create keeps it off.  This header adds the one call that
 * says whether a launch carried it: a table that silently stayed off would cost its speed-up and change nothing else.
 *
 * Kept apart from rt_abi.h, whose text is pinned: this header includes it and adds one call.
 */
#ifndef RT_PRIMARY_ABI_H
#define RT_PRIMARY_ABI_H

#include "rt_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 if the most recent trace launch of the context (rt_render_frame / rt_render_frames / rt_adaptive_render_frames) carried the table
 * switched on — a scene without trees, no defocus, a finite camera, at most 32 spheres, 4 models and 16 triangles — 0 if it did not,
 * -1 before the first launch; RT_ERR_INVALID_ARG for a null context. */
int rt_debug_primary_table(const RtContext* ctx);

#ifdef __cplusplus
}
#endif

#endif
