"""Loader and context wrapper for libraytrace_hip.so (the product path).

There is no fallback: if the shared library is missing or no HIP device is
usable, this raises — rendering never silently runs anywhere else.
"""
import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RT_HIP_LIB") or os.path.join(_HERE, "lib", "libraytrace_hip.so")  # RT_HIP_LIB: A/B builds

# every symbol include/rt_abi.h declares (tests check the library exports them all)
ABI_SYMBOLS = [
    "rt_create", "rt_destroy", "rt_last_error", "rt_set_stream", "rt_resize", "rt_set_partition", "rt_local_rows",
    "rt_local_to_global_row", "rt_bind_render_targets", "rt_get_render_targets", "rt_upload_scene", "rt_update_models",
    "rt_update_spheres", "rt_set_params", "rt_reset_accumulation", "rt_render_frame", "rt_render_frames",
    "rt_synchronize", "rt_get_frame", "rt_read_frame", "rt_read_accumulated", "rt_display", "rt_display_srgb8",
    "rt_write_accumulated", "rt_timer_begin", "rt_timer_end",
    "rt_enable_stats", "rt_reset_counters", "rt_get_counters", "rt_build_bvh", "rt_build_bvh_mt", "rt_build_bvh_gpu", "rt_build_bvh_gpu_release", "rt_camera_view_params", "rt_version",
    "rt_debug_intersect", "rt_debug_math_eval", "rt_debug_phase_profile", "rt_build_bvh_gpu_batch",
    "rt_flush", "rt_validate_scene", "rt_debug_layout", "rt_debug_layout_free", "rt_debug_fused_frames_cap",
    "rt_create_multi", "rt_destroy_multi", "rt_multi_count", "rt_multi_context", "rt_multi_resize", "rt_multi_upload_scene",
    "rt_multi_update_models", "rt_multi_update_spheres", "rt_multi_set_params", "rt_multi_reset_accumulation",
    "rt_multi_render_frame", "rt_multi_render_frames", "rt_multi_synchronize", "rt_gather_accumulated", "rt_gather_frame",
    "rt_multi_get_counters", "rt_multi_last_gather_ms", "rt_multi_peer_access", "rt_gather_accumulated_to_device", "rt_gather_frame_to_device",
    "rt_gather_rccl",
]
# every symbol include/rt_cost.h declares (kept apart: ABI_SYMBOLS mirrors rt_abi.h alone)
COST_SYMBOLS = ["rt_render_cost"]
# include/rt_held_back.h (test hooks; its third declaration restates rt_multi_context of rt_abi.h)
HELD_BACK_SYMBOLS = ["rt_debug_pending_frames", "rt_debug_multi_pending_frames"]
# include/rt_primary.h
PRIMARY_SYMBOLS = ["rt_debug_primary_table"]
# include/rt_tile_cand.h
TILE_CAND_SYMBOLS = ["rt_debug_tile_cand"]
# include/rt_tile_tri.h (which include/rt_tile_cand.h includes)
TILE_TRI_SYMBOLS = ["rt_debug_tile_tri"]
# every symbol include/rt_aov.h declares
AOV_SYMBOLS = ["rt_render_aov", "rt_render_aov_to_device"]
# every symbol include/rt_denoise.h declares
DENOISE_SYMBOLS = ["rt_denoise_default_params", "rt_denoise_buffers", "rt_denoise", "rt_denoise_to_device"]
# every symbol include/rt_reproject.h declares
REPROJECT_SYMBOLS = ["rt_reproject_default_params", "rt_reproject_buffers", "rt_reproject_accumulated", "rt_resolve_buffers", "rt_resolve",
                     "rt_resolve_to_device"]
# every symbol include/rt_motion.h declares
MOTION_SYMBOLS = ["rt_render_aov_centre", "rt_render_aov_centre_to_device", "rt_motion_from_scene", "rt_reproject_buffers_moving",
                  "rt_reproject_accumulated_moving"]
# every symbol include/rt_variance.h declares
VARIANCE_SYMBOLS = ["rt_denoise_variance_default_params", "rt_moments_update_buffers", "rt_denoise_variance_buffers", "rt_variance_update",
                    "rt_variance_reset", "rt_variance_carry", "rt_variance_read_moments", "rt_variance_moments_to_device", "rt_denoise_variance",
                    "rt_denoise_variance_to_device"]
# every symbol include/rt_adaptive.h declares
ADAPTIVE_SYMBOLS = ["rt_adaptive_default_params", "rt_adaptive_select_buffers", "rt_adaptive_select", "rt_adaptive_set_tiles", "rt_adaptive_read_tiles",
                    "rt_adaptive_read_tile_error", "rt_adaptive_render_frames"]
# every symbol include/rt_query.h declares
QUERY_SYMBOLS = ["rt_query_closest", "rt_query_closest_buffers", "rt_query_occluded", "rt_query_occluded_buffers"]
# every symbol include/rt_radiance.h declares
RADIANCE_SYMBOLS = ["rt_radiance_trace", "rt_radiance_trace_buffers"]
# every symbol include/rt_nee.h declares
NEE_SYMBOLS = ["rt_nee_trace", "rt_nee_trace_buffers", "rt_nee_light_count", "rt_debug_light_table", "rt_debug_light_table_free"]
# every symbol include/rt_mis.h declares
MIS_SYMBOLS = ["rt_mis_trace", "rt_debug_light_map", "rt_debug_light_map_free"]
# RtPixelCost (include/rt_cost.h): the eight uint32 columns of HipTracer.render_cost, in order
COST_FIELDS = ("segments", "innerSteps", "leafSteps", "triTests", "primaryInnerSteps", "primaryLeafSteps", "primaryTriTests", "firstHit")


class HipApi(abi.CApi):
    _EXTRA = {
        "create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
        "set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
        "set_partition": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
        "local_rows": (C.c_int, [C.c_void_p]),
        "local_to_global_row": (C.c_int, [C.c_void_p, C.c_int]),
        "bind_render_targets": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
        "get_render_targets": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
        "synchronize": (C.c_int, [C.c_void_p]),
        "flush": (C.c_int, [C.c_void_p]),
        "timer_begin": (C.c_int, [C.c_void_p]),
        "timer_end": (C.c_int, [C.c_void_p]),
        "enable_stats": (C.c_int, [C.c_void_p, C.c_int]),
        "build_bvh_mt": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                   C.POINTER(C.c_int), C.c_void_p, C.POINTER(abi.RtBvhStats)]),
        "build_bvh_gpu": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                    C.POINTER(C.c_int), C.c_void_p, C.POINTER(abi.RtBvhStats)]),
        "build_bvh_gpu_release": (None, []),
        "build_bvh_gpu_batch": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
        "validate_scene": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
        "debug_layout": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_char_p, C.c_void_p]),
        "debug_layout_free": (None, [C.c_void_p]),
        "debug_fused_frames_cap": (C.c_int, [C.c_void_p]),
        "debug_pending_frames": (C.c_int, [C.c_void_p]),
        "debug_multi_pending_frames": (C.c_int, [C.c_void_p]),
        "debug_intersect": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
        "debug_math_eval": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
        "debug_phase_profile": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
        "create_multi": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]),
        "destroy_multi": (None, [C.c_void_p]),
        "multi_count": (C.c_int, [C.c_void_p]),
        "multi_context": (C.c_void_p, [C.c_void_p, C.c_int]),
        "multi_resize": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
        "multi_upload_scene": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
        "multi_update_models": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
        "multi_update_spheres": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
        "multi_set_params": (C.c_int, [C.c_void_p, C.POINTER(abi.RtParams)]),
        "multi_reset_accumulation": (C.c_int, [C.c_void_p]),
        "multi_render_frame": (C.c_int, [C.c_void_p]),
        "multi_render_frames": (C.c_int, [C.c_void_p, C.c_int]),
        "multi_synchronize": (C.c_int, [C.c_void_p]),
        "gather_accumulated": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
        "gather_frame": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
        "multi_get_counters": (C.c_int, [C.c_void_p, C.POINTER(abi.RtCounters)]),
        "multi_last_gather_ms": (C.c_double, [C.c_void_p]),
        "multi_peer_access": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "gather_accumulated_to_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
        "gather_frame_to_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
        "gather_rccl": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
        "render_cost": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
        "render_aov": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
        "render_aov_to_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
        "denoise_default_params": (C.c_int, [C.POINTER(abi.RtDenoiseParams)]),
        "denoise_buffers": (C.c_int, [C.c_void_p, C.POINTER(abi.RtDenoiseParams), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
        "denoise": (C.c_int, [C.c_void_p, C.POINTER(abi.RtDenoiseParams), C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
        "denoise_to_device": (C.c_int, [C.c_void_p, C.POINTER(abi.RtDenoiseParams), C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
        "reproject_default_params": (C.c_int, [C.POINTER(abi.RtReprojectParams)]),
        "reproject_buffers": (C.c_int, [C.c_void_p, C.POINTER(abi.RtReprojectParams), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
        "reproject_accumulated": (C.c_int, [C.c_void_p, C.POINTER(abi.RtReprojectParams), C.c_void_p, C.c_int, C.c_void_p]),
        "resolve_buffers": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
        "resolve": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
        "resolve_to_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
        "render_aov_centre": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
        "render_aov_centre_to_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
        "motion_from_scene": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
        "reproject_buffers_moving": (C.c_int, [C.c_void_p, C.POINTER(abi.RtReprojectParams), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                               C.c_void_p]),
        "reproject_accumulated_moving": (C.c_int, [C.c_void_p, C.POINTER(abi.RtReprojectParams), C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
        "denoise_variance_default_params": (C.c_int, [C.POINTER(abi.RtVarianceDenoiseParams)]),
        "moments_update_buffers": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
        "denoise_variance_buffers": (C.c_int, [C.c_void_p, C.POINTER(abi.RtVarianceDenoiseParams), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
        "variance_update": (C.c_int, [C.c_void_p]),
        "variance_reset": (C.c_int, [C.c_void_p]),
        "variance_carry": (C.c_int, [C.c_void_p, C.POINTER(abi.RtReprojectParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
        "variance_read_moments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
        "variance_moments_to_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
        "denoise_variance": (C.c_int, [C.c_void_p, C.POINTER(abi.RtVarianceDenoiseParams), C.c_int, C.c_void_p, C.c_size_t]),
        "denoise_variance_to_device": (C.c_int, [C.c_void_p, C.POINTER(abi.RtVarianceDenoiseParams), C.c_int, C.c_void_p, C.c_size_t]),
        "adaptive_default_params": (C.c_int, [C.POINTER(abi.RtAdaptiveParams)]),
        "adaptive_select_buffers": (C.c_int, [C.c_void_p, C.POINTER(abi.RtAdaptiveParams), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
        "adaptive_select": (C.c_int, [C.c_void_p, C.POINTER(abi.RtAdaptiveParams), C.POINTER(abi.RtAdaptiveResult)]),
        "adaptive_set_tiles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
        "adaptive_read_tiles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
        "adaptive_read_tile_error": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
        "adaptive_render_frames": (C.c_int, [C.c_void_p, C.c_int]),
        "query_closest": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
        "query_closest_buffers": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
        "query_occluded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
        "query_occluded_buffers": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
        "radiance_trace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
        "radiance_trace_buffers": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
        "nee_trace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
        "nee_trace_buffers": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
        "nee_light_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "debug_light_table": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(abi.RtLightTableDump)]),
        "debug_light_table_free": (None, [C.POINTER(abi.RtLightTableDump)]),
        "mis_trace": (C.c_int, [C.POINTER(abi.MisBatch)]),
        "debug_light_map": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(abi.RtLightMapDump)]),
        "debug_light_map_free": (None, [C.POINTER(abi.RtLightMapDump)]),
    }

    def __init__(self, path=LIB_PATH):
        if not os.path.exists(path):
            raise FileNotFoundError(
                f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        super().__init__(path, "rt_")
        for name, (res, args) in self._EXTRA.items():
            self._bind(name, res, args)

    def validate_scene_arrays(self, models, triangles, nodes, spheres=None):
        """rt_validate_scene: the host half of rt_upload_scene (no device needed).  Returns {n_pairs, max_height, flat, n_filtered,
        prepare_ms}; raises RtError with the status and message rt_upload_scene would give."""
        m, nm = abi._ptr(models, abi.model_dtype)
        t, nt = abi._ptr(triangles, abi.triangle_dtype)
        n, nn = abi._ptr(nodes, abi.node_dtype)
        sp, ns = abi._ptr(spheres, abi.sphere_dtype)
        class _Info(C.Structure):
            _fields_ = [("n_pairs", C.c_int32), ("max_height", C.c_int32), ("flat", C.c_int32), ("n_filtered", C.c_int32), ("prepare_ms", C.c_float)]
        info = _Info()
        rc = self.validate_scene(m.ctypes.data if nm else None, nm, t.ctypes.data if nt else None, nt,
                                 n.ctypes.data if nn else None, nn, sp.ctypes.data if ns else None, ns, C.byref(info))
        if rc != abi.RT_OK:
            raise abi.RtError(rc, (self.last_error(None) or b"").decode(errors="replace"))
        return {k: getattr(info, k) for k, _ in _Info._fields_}

    def light_table_arrays(self, models, triangles, spheres=None):
        """rt_debug_light_table (include/rt_nee.h): the light table rt_nee_trace would sample for these arrays (no device
        needed), as numpy copies: {entries (abi.LIGHT_ENTRY_DTYPE), cdf (float32), n_sphere_entries, n_triangle_entries}."""
        m, nm = abi._ptr(models, abi.model_dtype)
        t, nt = abi._ptr(triangles, abi.triangle_dtype)
        sp, ns = abi._ptr(spheres, abi.sphere_dtype)
        d = abi.RtLightTableDump()
        rc = self.debug_light_table(m.ctypes.data if nm else None, nm, t.ctypes.data if nt else None, nt, sp.ctypes.data if ns else None, ns, C.byref(d))
        if rc != abi.RT_OK:
            raise abi.RtError(rc, (self.last_error(None) or b"").decode(errors="replace"))
        try:
            n = d.n_entries
            entries = np.frombuffer((C.c_char * (n * 80)).from_address(d.entries), dtype=abi.LIGHT_ENTRY_DTYPE).copy() if n else np.zeros(0, dtype=abi.LIGHT_ENTRY_DTYPE)
            cdf = np.frombuffer((C.c_char * (n * 4)).from_address(d.cdf), dtype=np.float32).copy() if n else np.zeros(0, dtype=np.float32)
            return {"entries": entries, "cdf": cdf, "n_sphere_entries": int(d.n_sphere_entries), "n_triangle_entries": int(d.n_triangle_entries)}
        finally:
            self.debug_light_table_free(C.byref(d))

    def light_map_arrays(self, models, triangles, spheres=None):
        """rt_debug_light_map (include/rt_mis.h): the reverse map of the light table of these arrays (no device needed), as numpy
        copies: {objects (uint32 per object), triangles (uint32 words), n_entries}; abi.MIS_NO_ENTRY = no entry."""
        m, nm = abi._ptr(models, abi.model_dtype)
        t, nt = abi._ptr(triangles, abi.triangle_dtype)
        sp, ns = abi._ptr(spheres, abi.sphere_dtype)
        d = abi.RtLightMapDump()
        rc = self.debug_light_map(m.ctypes.data if nm else None, nm, t.ctypes.data if nt else None, nt, sp.ctypes.data if ns else None, ns, C.byref(d))
        if rc != abi.RT_OK:
            raise abi.RtError(rc, (self.last_error(None) or b"").decode(errors="replace"))
        try:
            def words(ptr, n):
                return np.frombuffer((C.c_char * (n * 4)).from_address(ptr), dtype=np.uint32).copy() if n else np.zeros(0, dtype=np.uint32)
            return {"objects": words(d.objects, d.n_objects), "triangles": words(d.triangles, d.n_triangle_words), "n_entries": int(d.n_entries)}
        finally:
            self.debug_light_map_free(C.byref(d))

    def layout_arrays(self, models, triangles, nodes, layout=None):
        """rt_debug_layout: the device-memory layout rt_upload_scene would produce (no device needed), as numpy copies:
        {pair_space, tri_space (None: arena), norm_space (uint8), big_leaves (n,2), root_codes, tri_base, arena, used}."""
        m, nm = abi._ptr(models, abi.model_dtype)
        t, nt = abi._ptr(triangles, abi.triangle_dtype)
        n, nn = abi._ptr(nodes, abi.node_dtype)

        class _Dump(C.Structure):
            _fields_ = [("pair_space", C.c_void_p), ("pair_bytes", C.c_size_t), ("tri_space", C.c_void_p), ("tri_bytes", C.c_size_t),
                        ("norm_space", C.c_void_p), ("norm_bytes", C.c_size_t), ("big_leaves", C.c_void_p), ("n_big_leaves", C.c_size_t),
                        ("root_codes", C.c_void_p), ("tri_base", C.c_void_p), ("n_models", C.c_int32), ("arena", C.c_int32), ("used", C.c_char * 64)]
        d = _Dump()
        rc = self.debug_layout(m.ctypes.data if nm else None, nm, t.ctypes.data if nt else None, nt, n.ctypes.data if nn else None, nn,
                               layout.encode() if layout is not None else None, C.byref(d))
        if rc != abi.RT_OK:
            raise abi.RtError(rc, (self.last_error(None) or b"").decode(errors="replace"))

        def arr(ptr, count, dtype):
            if not ptr or not count:
                return np.zeros(0, dtype=dtype)
            return np.frombuffer((C.c_char * (count * np.dtype(dtype).itemsize)).from_address(ptr), dtype=dtype).copy()
        try:
            return {"pair_space": arr(d.pair_space, d.pair_bytes, np.uint8), "tri_space": None if d.arena else arr(d.tri_space, d.tri_bytes, np.uint8),
                    "norm_space": arr(d.norm_space, d.norm_bytes, np.uint8), "big_leaves": arr(d.big_leaves, 2 * d.n_big_leaves, np.uint32).reshape(-1, 2),
                    "root_codes": arr(d.root_codes, d.n_models, np.uint32), "tri_base": arr(d.tri_base, d.n_models, np.int32),
                    "arena": bool(d.arena), "used": d.used.decode()}
        finally:
            self.debug_layout_free(C.byref(d))

    def build_bvh_arrays_mt(self, verts, normals, indices, quality=abi.BVH_QUALITY_HIGH, threads=0):
        """rt_build_bvh_mt: same output as build_bvh_arrays, on `threads` host threads."""
        verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
        normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        indices = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1)
        ntri = len(indices) // 3
        nodes = np.zeros(2 * max(1, ntri), dtype=abi.node_dtype)
        tris = np.zeros(ntri, dtype=abi.triangle_dtype)
        n_nodes = C.c_int(0)
        stats = abi.RtBvhStats()
        rc = self.build_bvh_mt(verts.ctypes.data, normals.ctypes.data, len(verts), indices.ctypes.data, len(indices),
                               int(quality), int(threads), nodes.ctypes.data, C.byref(n_nodes), tris.ctypes.data, C.byref(stats))
        if rc != abi.RT_OK:
            raise abi.RtError(rc, "build_bvh_mt failed")
        return nodes[: n_nodes.value].copy(), tris, stats.as_dict()

    def build_bvh_arrays_gpu(self, verts, normals, indices, quality=abi.BVH_QUALITY_HIGH, device_id=0):
        """rt_build_bvh_gpu: same output as build_bvh_arrays, built on the GPU."""
        verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
        normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        indices = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1)
        ntri = len(indices) // 3
        nodes = np.zeros(2 * max(1, ntri), dtype=abi.node_dtype)
        tris = np.zeros(ntri, dtype=abi.triangle_dtype)
        n_nodes = C.c_int(0)
        stats = abi.RtBvhStats()
        rc = self.build_bvh_gpu(int(device_id), verts.ctypes.data, normals.ctypes.data, len(verts), indices.ctypes.data, len(indices),
                                int(quality), nodes.ctypes.data, C.byref(n_nodes), tris.ctypes.data, C.byref(stats))
        if rc != abi.RT_OK:
            raise abi.RtError(rc, "build_bvh_gpu failed")
        return nodes[: n_nodes.value].copy(), tris, stats.as_dict()

    def build_bvh_arrays_gpu_batch(self, meshes, quality=abi.BVH_QUALITY_HIGH, device_id=0):
        """rt_build_bvh_gpu_batch: [(verts, normals, indices), ...] -> (nodes, triangles, [(nodeOffset, triOffset, stats)]) — the
        concatenated arrays of CreateAllMeshData, written in place by the library (no per-mesh copies on this side)."""
        n = len(meshes)
        vs = [np.ascontiguousarray(m[0], dtype=np.float32).reshape(-1, 3) for m in meshes]
        ns = [np.ascontiguousarray(m[1], dtype=np.float32).reshape(-1, 3) for m in meshes]
        ix = [np.ascontiguousarray(m[2], dtype=np.int32).reshape(-1) for m in meshes]
        ntri = [len(i) // 3 for i in ix]
        nodes = np.empty(sum(2 * max(1, t) for t in ntri), dtype=abi.node_dtype)
        tris = np.empty(sum(ntri), dtype=abi.triangle_dtype)
        ptrs = lambda arrs: (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        ints = lambda vals: (C.c_int * n)(*vals)
        n_nodes, node_off, tri_off = ints([0] * n), ints([0] * n), ints([0] * n)
        stats = (abi.RtBvhStats * n)()
        rc = self.build_bvh_gpu_batch(int(device_id), n, ptrs(vs), ptrs(ns), ints([len(v) for v in vs]), ptrs(ix), ints([len(i) for i in ix]),
                                      int(quality), nodes.ctypes.data, n_nodes, node_off, tris.ctypes.data, tri_off, stats)
        if rc != abi.RT_OK:
            raise abi.RtError(rc, "build_bvh_gpu_batch failed")
        total = (node_off[n - 1] + n_nodes[n - 1]) if n else 0
        return nodes[:total], tris, [(node_off[k], tri_off[k], stats[k].as_dict()) for k in range(n)]

    def denoise_params(self, **fields):
        """rt_denoise_default_params, with `fields` (iterations, sigmaColour, sigmaNormal, sigmaPlane, demodulate, scale) set on top."""
        p = abi.RtDenoiseParams()
        rc = self.denoise_default_params(C.byref(p))
        if rc != abi.RT_OK:
            raise abi.RtError(rc, "rt_denoise_default_params failed")
        for k, v in fields.items():
            if k not in dict(abi.RtDenoiseParams._fields_):
                raise TypeError(f"RtDenoiseParams has no field {k!r}")
            setattr(p, k, v)
        return p

    def variance_denoise_params(self, **fields):
        """rt_denoise_variance_default_params, with `fields` (iterations, sigmaLuminance, sigmaNormal, sigmaPlane, demodulate, scale,
        unknownVariance) set on top."""
        p = abi.RtVarianceDenoiseParams()
        rc = self.denoise_variance_default_params(C.byref(p))
        if rc != abi.RT_OK:
            raise abi.RtError(rc, "rt_denoise_variance_default_params failed")
        for k, v in fields.items():
            if k not in dict(abi.RtVarianceDenoiseParams._fields_):
                raise TypeError(f"RtVarianceDenoiseParams has no field {k!r}")
            if k == "reserved":
                p.reserved[:] = [int(x) for x in v]
            else:
                setattr(p, k, v)
        return p

    def adaptive_params(self, **fields):
        """rt_adaptive_default_params, with `fields` (threshold, darkFloor, minFrames, maxFrames) set on top."""
        p = abi.RtAdaptiveParams()
        rc = self.adaptive_default_params(C.byref(p))
        if rc != abi.RT_OK:
            raise abi.RtError(rc, "rt_adaptive_default_params failed")
        for k, v in fields.items():
            if k not in dict(abi.RtAdaptiveParams._fields_):
                raise TypeError(f"RtAdaptiveParams has no field {k!r}")
            if k == "reserved":
                p.reserved[:] = [int(x) for x in v]
            else:
                setattr(p, k, v)
        return p

    def reproject_params(self, prev_params=None, **fields):
        """rt_reproject_default_params, with the previous camera taken from `prev_params` (the RtParams of the view that is being left)
        and `fields` (prevViewParams, prevCamLocalToWorld, maxPlaneDistance, minNormalDot, maxHistory, flags) set on top."""
        p = abi.RtReprojectParams()
        rc = self.reproject_default_params(C.byref(p))
        if rc != abi.RT_OK:
            raise abi.RtError(rc, "rt_reproject_default_params failed")
        if prev_params is not None:
            p.prevViewParams[:] = list(prev_params.viewParams)
            p.prevCamLocalToWorld[:] = list(prev_params.camLocalToWorld)
        for k, v in fields.items():
            if k not in dict(abi.RtReprojectParams._fields_):
                raise TypeError(f"RtReprojectParams has no field {k!r}")
            if k in ("prevViewParams", "prevCamLocalToWorld"):
                getattr(p, k)[:] = [float(x) for x in v]
            else:
                setattr(p, k, v)
        return p

    def motion_table(self, prev_spheres, cur_spheres, prev_models, cur_models):
        """rt_motion_from_scene (include/rt_motion.h): the per-object table between two states of one scene, an array of
        abi.OBJECT_MOTION_DTYPE with the object numbering of RtPixelAov.object (spheres first, then models).  Host code: no device."""
        ps, n_ps = abi._ptr(prev_spheres, abi.sphere_dtype)
        cs, n_cs = abi._ptr(cur_spheres, abi.sphere_dtype)
        pm, n_pm = abi._ptr(prev_models, abi.model_dtype)
        cm, n_cm = abi._ptr(cur_models, abi.model_dtype)
        if n_ps != n_cs or n_pm != n_cm:
            raise ValueError("the two states of the scene differ in their number of spheres or models")
        out = np.zeros(n_ps + n_pm, dtype=abi.OBJECT_MOTION_DTYPE)
        rc = self.motion_from_scene(ps.ctypes.data if n_ps else None, cs.ctypes.data if n_ps else None, n_ps, pm.ctypes.data if n_pm else None,
                                    cm.ctypes.data if n_pm else None, n_pm, out.ctypes.data if out.size else None)
        if rc != abi.RT_OK:
            raise abi.RtError(rc, (self.last_error(None) or b"").decode(errors="replace"))
        return out

    def create_tracer(self, device_id=0):
        h = C.c_void_p()
        rc = self.create(device_id, C.byref(h))
        if rc != abi.RT_OK:
            msg = self.last_error(None)
            raise abi.RtError(rc, msg.decode() if msg else "rt_create failed")
        return HipTracer(self, h.value)

    def create_multi_tracer(self, device_ids):
        return MultiTracer(self, list(device_ids))


class MultiTracer:
    """rt_create_multi: n contexts (one per device id) in THIS process, cyclic 8-row strips, gather at
    readback.  Quacks like a Tracer for the RayComputeManager mirror (resize / upload_scene / update_models /
    set_params / reset_accumulation / render_frame(s) / read_accumulated)."""

    def __init__(self, api, device_ids):
        self.api = api
        ids = (C.c_int * len(device_ids))(*device_ids)
        h = C.c_void_p()
        rc = api.create_multi(ids, len(device_ids), C.byref(h))
        if rc != abi.RT_OK:
            msg = api.last_error(None)
            raise abi.RtError(rc, msg.decode() if msg else "rt_create_multi failed")
        self.h = h.value
        self.size = (0, 0)

    def _check(self, rc):
        if rc != abi.RT_OK:
            msg = self.api.last_error(self.api.multi_context(self.h, 0))
            raise abi.RtError(rc, msg.decode() if msg else "")

    def close(self):
        if self.h:
            self.api.destroy_multi(self.h)
            self.h = None

    def context(self, i):
        """Borrowed per-device context (owned by the multi handle: closing it is a no-op)."""
        t = _BorrowedTracer(self.api, self.api.multi_context(self.h, i))
        t.width, t.height = self.size
        return t

    def resize(self, w, h):
        self._check(self.api.multi_resize(self.h, w, h))
        self.size = (w, h)

    def upload_scene(self, models, triangles, nodes, spheres=None):
        m, nm = abi._ptr(models, abi.model_dtype)
        t, nt = abi._ptr(triangles, abi.triangle_dtype)
        n, nn = abi._ptr(nodes, abi.node_dtype)
        sp, ns = abi._ptr(spheres, abi.sphere_dtype)
        self._check(self.api.multi_upload_scene(
            self.h, m.ctypes.data if nm else None, nm, t.ctypes.data if nt else None, nt,
            n.ctypes.data if nn else None, nn, sp.ctypes.data if ns else None, ns))

    def update_models(self, models):
        m, nm = abi._ptr(models, abi.model_dtype)
        self._check(self.api.multi_update_models(self.h, m.ctypes.data if nm else None, nm))

    def update_spheres(self, spheres):
        sp, ns = abi._ptr(spheres, abi.sphere_dtype)
        self._check(self.api.multi_update_spheres(self.h, sp.ctypes.data if ns else None, ns))

    def set_params(self, params):
        params.abi_version = abi.RT_ABI_VERSION
        params.struct_size = C.sizeof(abi.RtParams)
        self._check(self.api.multi_set_params(self.h, C.byref(params)))

    def reset_accumulation(self):
        self._check(self.api.multi_reset_accumulation(self.h))

    def render_frame(self):
        self._check(self.api.multi_render_frame(self.h))

    def render_frames(self, n):
        self._check(self.api.multi_render_frames(self.h, n))

    def synchronize(self):
        self._check(self.api.multi_synchronize(self.h))

    def _gather(self, fn):
        w, h = self.size
        out = np.zeros((h, w, 4), dtype=np.float32)
        self._check(fn(self.h, out.ctypes.data, out.nbytes))
        return out

    def read_accumulated(self):
        return self._gather(self.api.gather_accumulated)

    def read_frame(self):
        return self._gather(self.api.gather_frame)

    def gather_accumulated_to_device(self, root, device_ptr, nbytes):
        """rt_gather_accumulated_to_device: the image lands in device memory of context `root`'s GPU (e.g. a torch tensor)."""
        self._check(self.api.gather_accumulated_to_device(self.h, int(root), device_ptr, nbytes))

    def gather_frame_to_device(self, root, device_ptr, nbytes):
        self._check(self.api.gather_frame_to_device(self.h, int(root), device_ptr, nbytes))

    def last_gather_ms(self):
        return float(self.api.multi_last_gather_ms(self.h))

    def pending_frames(self):
        """rt_debug_multi_pending_frames (test hook): the most frames any context holds back right now."""
        return self.api.debug_multi_pending_frames(self.h)

    def counters(self):
        c = abi.RtCounters()
        self._check(self.api.multi_get_counters(self.h, C.byref(c)))
        return c.as_dict()

    def render_cost(self, frame):
        """rt_render_cost on every context, assembled into the whole image: (H, W, 8) uint32, rows bottom-up (COST_FIELDS)."""
        _, h = self.size
        out = None
        for i in range(self.api.multi_count(self.h)):
            ctx = self.context(i)
            part = scatter_rows(ctx.render_cost(frame), ctx.local_to_global_rows(), h)
            out = part if out is None else out + part  # (the contexts' rows are disjoint: elsewhere each part is 0)
        return out

    def render_aov(self, frame):
        """rt_render_aov on every context, assembled into the whole image: (H, W) records of abi.AOV_DTYPE, rows bottom-up."""
        w, h = self.size
        out = np.zeros((h, w), dtype=abi.AOV_DTYPE)
        for i in range(self.api.multi_count(self.h)):
            ctx = self.context(i)
            out[ctx.local_to_global_rows()] = ctx.render_aov(frame)  # (the contexts' rows are disjoint)
        return out


    def _needs_whole_image(self, what):
        raise abi.RtError(abi.RT_ERR_STATE, f"{what}: every context of a MultiTracer owns part of the image; gather the image and the AOV records "
                                            "of all parts onto one device (gather_accumulated_to_device), then use the *_buffers call of one context")

    def reproject_accumulated(self, *args, **kwargs):
        self._needs_whole_image("reproject_accumulated")

    def reproject_accumulated_moving(self, *args, **kwargs):
        self._needs_whole_image("reproject_accumulated_moving")

    def render_aov_centre(self):
        """rt_render_aov_centre on every context, assembled into the whole image like render_aov."""
        w, h = self.size
        out = np.zeros((h, w), dtype=abi.AOV_DTYPE)
        for i in range(self.api.multi_count(self.h)):
            ctx = self.context(i)
            out[ctx.local_to_global_rows()] = ctx.render_aov_centre()
        return out

    def resolve(self, *args, **kwargs):
        self._needs_whole_image("resolve")

    def resolve_to_device(self, *args, **kwargs):
        self._needs_whole_image("resolve_to_device")


class HipTracer(abi.Tracer):
    """An RtContext on one MI355X."""

    def set_stream(self, stream_ptr):
        self._check(self.api.set_stream(self.h, stream_ptr))

    def set_partition(self, strip_rows, part_index, part_count):
        self._check(self.api.set_partition(self.h, strip_rows, part_index, part_count))

    def local_rows(self):
        return self.api.local_rows(self.h)

    def local_to_global_rows(self):
        n = self.local_rows()
        return np.array([self.api.local_to_global_row(self.h, i) for i in range(n)], dtype=np.int64)

    def bind_render_targets(self, frame_ptr, accum_ptr):
        self._check(self.api.bind_render_targets(self.h, frame_ptr, accum_ptr))

    def render_targets(self):
        f, a = C.c_void_p(), C.c_void_p()
        self._check(self.api.get_render_targets(self.h, C.byref(f), C.byref(a)))
        return f.value, a.value

    def gather_rccl(self, nccl_comm, root, device_ptr, nbytes, accumulated=True):
        """rt_gather_rccl: this rank's packed tile to `root` over the caller's ncclComm_t (RCCL), de-interleaved into the whole image
        at device_ptr on root (others pass None / 0)."""
        self._check(self.api.gather_rccl(self.h, nccl_comm, int(root), 1 if accumulated else 0, device_ptr, nbytes))

    def fused_frames_cap(self):
        return self.api.debug_fused_frames_cap(self.h)

    def pending_frames(self):
        """rt_debug_pending_frames (test hook): frames counted by render_frame but not launched yet."""
        return self.api.debug_pending_frames(self.h)

    def primary_table(self):
        """rt_debug_primary_table: 1 / 0 = the last trace launch carried its table of ray-origin constants switched on / off, -1 = no launch yet"""
        # bound on first use: tools/ab_libs.py loads libraries of earlier commits, which do not have it, through this class
        fn = self.api.lib.rt_debug_primary_table
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p]
        return fn(self.h)

    def tile_cand(self):
        """rt_debug_tile_cand: 1 / 0 = the last trace launch read / did not read the per-tile table of sphere candidates, -1 = no launch yet"""
        fn = self.api.lib.rt_debug_tile_cand  # bound on first use, like primary_table
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p]
        return fn(self.h)

    def tile_tri(self):
        """rt_debug_tile_tri: 1 / 0 = the table the last trace launch read held / did not hold per-tile triangle masks, -1 = no launch yet"""
        fn = self.api.lib.rt_debug_tile_tri  # bound on first use, like primary_table
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p]
        return fn(self.h)

    def synchronize(self):
        self._check(self.api.synchronize(self.h))

    def flush(self):
        self._check(self.api.flush(self.h))

    def timer_begin(self):
        self._check(self.api.timer_begin(self.h))

    def timer_end(self):
        self._check(self.api.timer_end(self.h))

    def enable_stats(self, on=True):
        self._check(self.api.enable_stats(self.h, 1 if on else 0))

    def debug_intersect(self, origins, dirs):
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        out = np.zeros((len(o), 10), dtype=np.float32)
        self._check(self.api.debug_intersect(self.h, o.ctypes.data, d.ctypes.data, len(o), out.ctypes.data))
        return out

    PHASES = ["loop", "raygen", "spheres", "traverse_call", "model", "inner", "tri", "shade_hit", "sky", "sphere_roots", "glass", "refill"]

    def phase_profile(self):
        n = len(self.PHASES)
        out = np.zeros(3 * n + 1, dtype=np.uint64)
        self._check(self.api.debug_phase_profile(self.h, out.ctypes.data, len(out)))
        prof = {p: (int(out[2 * i]), int(out[2 * i + 1])) for i, p in enumerate(self.PHASES)}
        prof["filter_violations"] = (int(out[2 * n]), 0)
        # round 6: inner steps (lane-steps) served by the LDS top-of-tree cache, and taken while >= 48 lanes / >= 3/4 of >= 16 active lanes
        # of the wave stood on ONE node (the case for a scalar top-of-tree path)
        prof["inner_from_lds_cache"] = (int(out[2 * n + 1]), 0)
        prof["inner_on_one_node_48_lanes"] = (int(out[2 * n + 2]), 0)
        prof["inner_on_one_node_3_of_4_active"] = (int(out[2 * n + 3]), 0)
        return prof

    def render_cost(self, frame):
        """rt_render_cost: the work the rays of frame `frame` (>= 1) do per pixel of this context's rows, as a (local_rows, W, 8)
        uint32 array in rt_read_frame's order; the columns are COST_FIELDS.  Changes no state of the context."""
        out = np.zeros((max(self.local_rows(), 0), self.width, len(COST_FIELDS)), dtype=np.uint32)
        self._check(self.api.render_cost(self.h, int(frame), out.ctypes.data if out.size else None, out.nbytes))
        return out

    def render_aov(self, frame):
        """rt_render_aov (include/rt_aov.h): what camera ray 0 of frame `frame` (>= 1) hits first, per pixel of this context's rows:
        a (local_rows, W) array of abi.AOV_DTYPE (dst, normal, pos, hit, albedo, object, emission, triangle) in rt_read_frame's
        order.  A picked pixel is aov[y, x]["object"].  Changes no state of the context."""
        out = np.zeros((max(self.local_rows(), 0), self.width), dtype=abi.AOV_DTYPE)
        self._check(self.api.render_aov(self.h, int(frame), out.ctypes.data if out.size else None, out.nbytes))
        return out

    def render_aov_to_device(self, frame, ptr, nbytes):
        """rt_render_aov_to_device: the same records into device memory (e.g. a torch tensor's data_ptr(), local_rows * W * 64 bytes),
        enqueued on the stream the context renders on; complete after synchronize()."""
        self._check(self.api.render_aov_to_device(self.h, int(frame), ptr, int(nbytes)))

    def render_aov_centre(self):
        """rt_render_aov_centre (include/rt_motion.h): the records of the rays through the unjittered pixel centres, the same array as
        render_aov's; they depend on no frame counter, seed, defocus or jitter.  Changes no state of the context."""
        out = np.zeros((max(self.local_rows(), 0), self.width), dtype=abi.AOV_DTYPE)
        self._check(self.api.render_aov_centre(self.h, out.ctypes.data if out.size else None, out.nbytes))
        return out

    def render_aov_centre_to_device(self, ptr, nbytes):
        """rt_render_aov_centre_to_device: the same records into device memory, enqueued like render_aov_to_device."""
        self._check(self.api.render_aov_centre_to_device(self.h, ptr, int(nbytes)))

    def query_closest(self, rays):
        """rt_query_closest (include/rt_query.h): CalculateRayCollision for each of `rays` (n records of abi.RAY_DTYPE: origin, tmax, dir,
        reserved; the direction is used as given, not normalised) against the uploaded scene: n records of abi.RAYHIT_DTYPE (dst, normal,
        pos, hit, object, triangle, reserved).  abi.make_rays builds the input.  Changes no state of the context."""
        r = np.ascontiguousarray(rays, dtype=abi.RAY_DTYPE).reshape(-1)
        out = np.zeros(len(r), dtype=abi.RAYHIT_DTYPE)
        self._check(self.api.query_closest(self.h, r.ctypes.data if len(r) else None, len(r), out.ctypes.data if len(r) else None))
        return out

    def query_occluded(self, rays):
        """rt_query_occluded: per ray, 1 if it hits anything at a distance (in units of |dir|) strictly below its tmax, else 0: n uint32."""
        r = np.ascontiguousarray(rays, dtype=abi.RAY_DTYPE).reshape(-1)
        out = np.zeros(len(r), dtype=np.uint32)
        self._check(self.api.query_occluded(self.h, r.ctypes.data if len(r) else None, len(r), out.ctypes.data if len(r) else None))
        return out

    def query_closest_buffers(self, rays_ptr, n, hits_ptr):
        """rt_query_closest_buffers: the same on device memory (e.g. torch tensors' data_ptr(): n * 32 bytes of rays, n * 48 bytes of
        records, 16-byte aligned), enqueued on the stream the context renders on; complete after synchronize()."""
        self._check(self.api.query_closest_buffers(self.h, rays_ptr, int(n), hits_ptr))

    def query_occluded_buffers(self, rays_ptr, n, occluded_ptr):
        """rt_query_occluded_buffers: the answers (n uint32, 0 / 1) into device memory, enqueued like query_closest_buffers."""
        self._check(self.api.query_occluded_buffers(self.h, rays_ptr, int(n), occluded_ptr))

    def radiance_trace(self, rays):
        """rt_radiance_trace (include/rt_radiance.h): the reference's Trace for each of `rays` (n records of abi.PATHRAY_DTYPE: origin,
        unused, dir, rng; the direction is used as given, rng is the generator state the path starts with) against the uploaded scene
        under the parameters last set: n records of abi.RADIANCE_DTYPE (rgb, and rng = the state when Trace returned, to chain further
        samples).  abi.make_path_rays builds the input.  Changes no state of the context."""
        r = np.ascontiguousarray(rays, dtype=abi.PATHRAY_DTYPE).reshape(-1)
        out = np.zeros(len(r), dtype=abi.RADIANCE_DTYPE)
        self._check(self.api.radiance_trace(self.h, r.ctypes.data if len(r) else None, len(r), out.ctypes.data if len(r) else None))
        return out

    def radiance_trace_buffers(self, rays_ptr, n, out_ptr):
        """rt_radiance_trace_buffers: the same on device memory (e.g. torch tensors' data_ptr(): n * 32 bytes of rays, n * 16 bytes of
        records, 16-byte aligned), enqueued on the stream the context renders on; complete after synchronize()."""
        self._check(self.api.radiance_trace_buffers(self.h, rays_ptr, int(n), out_ptr))

    def radiance_trace_nee(self, rays):
        """rt_nee_trace (include/rt_nee.h): radiance_trace with one emitter of the scene sampled directly at every diffuse
        vertex (next-event estimation) — the same records, the same expectation per ray up to the cut at maxBounceCount (the header states it), less variance where small emitters light
        the scene.  Changes no state of the context."""
        r = np.ascontiguousarray(rays, dtype=abi.PATHRAY_DTYPE).reshape(-1)
        out = np.zeros(len(r), dtype=abi.RADIANCE_DTYPE)
        self._check(self.api.nee_trace(self.h, r.ctypes.data if len(r) else None, len(r), out.ctypes.data if len(r) else None))
        return out

    def radiance_trace_nee_buffers(self, rays_ptr, n, out_ptr):
        """rt_nee_trace_buffers: the same on device memory, enqueued like radiance_trace_buffers."""
        self._check(self.api.nee_trace_buffers(self.h, rays_ptr, int(n), out_ptr))

    def _mis_batch(self, memory, rays_ptr, n, out_ptr):
        b = abi.MisBatch()
        b.struct_size, b.memory, b.ctx, b.rays, b.out, b.n, b.reserved = C.sizeof(abi.MisBatch), memory, self.h, rays_ptr, out_ptr, int(n), 0
        return b

    def radiance_trace_mis(self, rays):
        """rt_mis_trace, host form (include/rt_mis.h): radiance_trace with one emitter sampled directly at every diffuse vertex that
        has a bounce left, combined with the cosine lobe by the balance heuristic — the same records, radiance_trace's expectation
        at every maxBounceCount, and every contribution at most T * Le.  Changes no state of the context."""
        r = np.ascontiguousarray(rays, dtype=abi.PATHRAY_DTYPE).reshape(-1)
        out = np.zeros(len(r), dtype=abi.RADIANCE_DTYPE)
        b = self._mis_batch(abi.MIS_HOST, r.ctypes.data if len(r) else None, len(r), out.ctypes.data if len(r) else None)
        self._check(self.api.mis_trace(C.byref(b)))
        return out

    def radiance_trace_mis_buffers(self, rays_ptr, n, out_ptr):
        """rt_mis_trace, device form: the same on device memory, enqueued like radiance_trace_buffers."""
        b = self._mis_batch(abi.MIS_DEVICE, rays_ptr, n, out_ptr)
        self._check(self.api.mis_trace(C.byref(b)))

    def nee_light_count(self):
        """rt_nee_light_count: (sphere entries, triangle entries) of the light table as the next radiance_trace_nee would use it."""
        ns, nt = C.c_int(0), C.c_int(0)
        self._check(self.api.nee_light_count(self.h, C.byref(ns), C.byref(nt)))
        return ns.value, nt.value

    def denoise(self, params=None, use_accumulated=True, aov_frame=1):
        """rt_denoise (include/rt_denoise.h): the context's accumulated image (or its last frame) through the edge-avoiding a-trous
        filter, guided by the AOV pass of frame `aov_frame`: a (rows, W, 4) float32 array, rows bottom-up.  `params`: an
        abi.RtDenoiseParams (default: api.denoise_params()); the accumulated image is a sum, so scale = 1 / frames.  Changes no state
        of the context."""
        p = params if params is not None else self.api.denoise_params()
        out = np.zeros((max(self.local_rows(), 0), self.width, 4), dtype=np.float32)
        self._check(self.api.denoise(self.h, C.byref(p), 1 if use_accumulated else 0, int(aov_frame), out.ctypes.data if out.size else None, out.nbytes))
        return out

    def denoise_to_device(self, ptr, nbytes, params=None, use_accumulated=True, aov_frame=1):
        """rt_denoise_to_device: the same image into device memory (e.g. a torch tensor's data_ptr(), rows * W * 16 bytes), enqueued on
        the stream the context renders on; complete after synchronize()."""
        p = params if params is not None else self.api.denoise_params()
        self._check(self.api.denoise_to_device(self.h, C.byref(p), 1 if use_accumulated else 0, int(aov_frame), ptr, int(nbytes)))

    def denoise_buffers(self, width, height, rgba_in_ptr, aov_ptr, rgba_out_ptr, params=None):
        """rt_denoise_buffers: the filter alone on caller-owned device memory (width x height RGBA32F in and out, width x height
        RtPixelAov records), enqueued on the stream the context renders on.  Needs no scene and no resize."""
        p = params if params is not None else self.api.denoise_params()
        self._check(self.api.denoise_buffers(self.h, C.byref(p), int(width), int(height), rgba_in_ptr, aov_ptr, rgba_out_ptr))

    def reproject_buffers(self, width, height, prev_rgba_ptr, prev_aov_ptr, cur_aov_ptr, out_rgba_ptr, params):
        """rt_reproject_buffers (include/rt_reproject.h): the reprojection alone on caller-owned device memory, enqueued on the stream the
        context renders on.  `params`: api.reproject_params(previous RtParams, ...).  Needs no scene and no resize."""
        self._check(self.api.reproject_buffers(self.h, C.byref(params), int(width), int(height), prev_rgba_ptr, prev_aov_ptr, cur_aov_ptr, out_rgba_ptr))

    def reproject_accumulated(self, params, prev_aov_ptr, aov_frame=1, cur_aov_out_ptr=None):
        """rt_reproject_accumulated: after set_params with the new camera, replace the accumulated image by its reprojection into the
        current view.  prev_aov_ptr: the device records of the view that was left (render_aov_to_device before the move);
        cur_aov_out_ptr: optional device memory that receives the current view's records.  Only enqueues."""
        self._check(self.api.reproject_accumulated(self.h, C.byref(params), prev_aov_ptr, int(aov_frame), cur_aov_out_ptr))

    def reproject_buffers_moving(self, width, height, prev_rgba_ptr, prev_aov_ptr, cur_aov_ptr, motion_ptr, n_objects, out_rgba_ptr, params):
        """rt_reproject_buffers_moving (include/rt_motion.h): reproject_buffers with a device table of n_objects abi.RtObjectMotion entries
        (api.motion_table, uploaded); motion_ptr may be None when n_objects == 0."""
        self._check(self.api.reproject_buffers_moving(self.h, C.byref(params), int(width), int(height), prev_rgba_ptr, prev_aov_ptr, cur_aov_ptr, motion_ptr,
                                                      int(n_objects), out_rgba_ptr))

    def reproject_accumulated_moving(self, params, prev_aov_ptr, aov_frame, motion_ptr, n_objects, cur_aov_out_ptr=None):
        """rt_reproject_accumulated_moving, in the C call's argument order: reproject_accumulated with the device table of the objects that
        moved since the previous view (after update_models / update_spheres and set_params).  aov_frame = abi.AOV_CENTRE: pixel-centre
        records, which prev_aov_ptr should then hold too (render_aov_centre_to_device, or the cur_aov_out_ptr of the last call).  Only
        enqueues."""
        self._check(self.api.reproject_accumulated_moving(self.h, C.byref(params), prev_aov_ptr, int(aov_frame), motion_ptr, int(n_objects), cur_aov_out_ptr))

    def resolve(self):
        """rt_resolve: the accumulated image divided per pixel by its own frame count (alpha): (rows, W, 4) float32, rows bottom-up; the
        alpha channel is the history length."""
        out = np.zeros((max(self.local_rows(), 0), self.width, 4), dtype=np.float32)
        self._check(self.api.resolve(self.h, out.ctypes.data if out.size else None, out.nbytes))
        return out

    def resolve_to_device(self, ptr, nbytes):
        """rt_resolve_to_device: the same image into device memory (rows * W * 16 bytes), enqueued on the stream the context renders on."""
        self._check(self.api.resolve_to_device(self.h, ptr, int(nbytes)))

    def resolve_buffers(self, width, height, rgba_sum_ptr, rgba_out_ptr):
        """rt_resolve_buffers: the per-pixel divide on caller-owned device memory (in place when both pointers are equal)."""
        self._check(self.api.resolve_buffers(self.h, int(width), int(height), rgba_sum_ptr, rgba_out_ptr))

    def variance_denoise_params(self, **fields):
        """api.variance_denoise_params: the defaults of rt_denoise_variance_default_params with `fields` set on top."""
        return self.api.variance_denoise_params(**fields)

    def moments_update_buffers(self, width, height, sum_ptr, snapshot_ptr, moments_ptr, rebase=False):
        """rt_moments_update_buffers (include/rt_variance.h): one batch — the sum's growth since the snapshot — into a moments image
        (sum of L, sum of L^2, 0, batches), all caller-owned device memory; rebase=True only copies the sum into the snapshot."""
        self._check(self.api.moments_update_buffers(self.h, int(width), int(height), sum_ptr, snapshot_ptr, moments_ptr, 1 if rebase else 0))

    def denoise_variance_buffers(self, width, height, rgba_in_ptr, moments_ptr, aov_ptr, rgba_out_ptr, params=None):
        """rt_denoise_variance_buffers: the variance-guided filter alone on caller-owned device memory.  Needs no scene and no resize."""
        p = params if params is not None else self.api.variance_denoise_params()
        self._check(self.api.denoise_variance_buffers(self.h, C.byref(p), int(width), int(height), rgba_in_ptr, moments_ptr, aov_ptr, rgba_out_ptr))

    def variance_update(self):
        """rt_variance_update: the frames rendered since the last update become one batch of the context's moments."""
        self._check(self.api.variance_update(self.h))

    def variance_reset(self):
        """rt_variance_reset: no batches; the snapshot is the accumulated image as it stands (after reset_accumulation / write_accumulated)."""
        self._check(self.api.variance_reset(self.h))

    def variance_carry(self, params, prev_aov_ptr, cur_aov_ptr, motion_ptr=None, n_objects=0):
        """rt_variance_carry: right after reproject_accumulated[_moving], with its parameters, its prev_aov_ptr and the records it wrote
        (cur_aov_out_ptr): the context's moments follow the accumulated image into the new view."""
        self._check(self.api.variance_carry(self.h, C.byref(params), prev_aov_ptr, cur_aov_ptr, motion_ptr, int(n_objects)))

    def read_moments(self):
        """rt_variance_read_moments: the context's moments, (rows, W, 4) float32, rows bottom-up: sum of L, sum of L^2, 0, batches."""
        out = np.zeros((max(self.local_rows(), 0), self.width, 4), dtype=np.float32)
        self._check(self.api.variance_read_moments(self.h, out.ctypes.data if out.size else None, out.nbytes))
        return out

    def moments_to_device(self, ptr, nbytes):
        """rt_variance_moments_to_device: the same image into device memory (rows * W * 16 bytes), enqueued."""
        self._check(self.api.variance_moments_to_device(self.h, ptr, int(nbytes)))

    def denoise_variance(self, params=None, aov_frame=1):
        """rt_denoise_variance: the accumulated image, resolved per pixel, through the variance-guided a-trous filter, steered by the
        context's moments and the AOV pass of frame `aov_frame`: (rows, W, 4) float32, rows bottom-up.  Changes no state."""
        p = params if params is not None else self.api.variance_denoise_params()
        out = np.zeros((max(self.local_rows(), 0), self.width, 4), dtype=np.float32)
        self._check(self.api.denoise_variance(self.h, C.byref(p), int(aov_frame), out.ctypes.data if out.size else None, out.nbytes))
        return out

    def denoise_variance_to_device(self, ptr, nbytes, params=None, aov_frame=1):
        """rt_denoise_variance_to_device: the same image into device memory (rows * W * 16 bytes), enqueued; complete after synchronize()."""
        p = params if params is not None else self.api.variance_denoise_params()
        self._check(self.api.denoise_variance_to_device(self.h, C.byref(p), int(aov_frame), ptr, int(nbytes)))

    def adaptive_params(self, **fields):
        """api.adaptive_params: the defaults of rt_adaptive_default_params with `fields` set on top."""
        return self.api.adaptive_params(**fields)

    def adaptive_select_buffers(self, width, height, sum_ptr, moments_ptr, tile_error_ptr, tiles_ptr, counts_ptr, params=None):
        """rt_adaptive_select_buffers (include/rt_adaptive.h): tile errors, the ordered list of active tiles and uint32[4] counts =
        (tiles_active, pixels_active, 0, 0), all caller-owned device memory.  Needs no scene and no resize; enqueued."""
        p = params if params is not None else self.api.adaptive_params()
        self._check(self.api.adaptive_select_buffers(self.h, C.byref(p), int(width), int(height), sum_ptr, moments_ptr, tile_error_ptr, tiles_ptr, counts_ptr))

    def adaptive_select(self, params=None):
        """rt_adaptive_select: the context's tiles whose error exceeds params.threshold become its current list.  Returns
        {tiles_total, tiles_active, pixels_active}.  Does not run variance_update."""
        p = params if params is not None else self.api.adaptive_params()
        out = abi.RtAdaptiveResult()
        self._check(self.api.adaptive_select(self.h, C.byref(p), C.byref(out)))
        return out.as_dict()

    def adaptive_set_tiles(self, tiles):
        """rt_adaptive_set_tiles: a list from the host (strictly increasing tile indices) in place of a selected one."""
        t = np.ascontiguousarray(tiles, dtype=np.uint32).reshape(-1)
        self._check(self.api.adaptive_set_tiles(self.h, t.ctypes.data if t.size else None, int(t.size)))

    def adaptive_tiles(self):
        """rt_adaptive_read_tiles: the current list, uint32, increasing."""
        n = C.c_int(0)
        self._check(self.api.adaptive_read_tiles(self.h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint32)
        if n.value:
            self._check(self.api.adaptive_read_tiles(self.h, out.ctypes.data, n.value, C.byref(n)))
        return out

    def adaptive_tile_error(self):
        """rt_adaptive_read_tile_error: (tilesY, tilesX) float32, the tile errors of the last adaptive_select (row 0 at the bottom)."""
        ty, tx = (max(self.local_rows(), 0) + 7) // 8, (self.width + 7) // 8
        out = np.zeros((ty, tx), dtype=np.float32)
        self._check(self.api.adaptive_read_tile_error(self.h, out.ctypes.data if out.size else None, out.nbytes))
        return out

    def adaptive_render_frames(self, n):
        """rt_adaptive_render_frames: frames Frame ... Frame + n - 1 of the current list's tiles; every other pixel keeps its bits."""
        self._check(self.api.adaptive_render_frames(self.h, int(n)))

    def debug_math_eval(self, op, x, y=None):
        x = np.ascontiguousarray(x, dtype=np.float32)
        y = np.ascontiguousarray(np.zeros_like(x) if y is None else y, dtype=np.float32)
        out = np.empty_like(x)
        self._check(self.api.debug_math_eval(self.h, int(op), x.ctypes.data, y.ctypes.data, out.ctypes.data, len(x)))
        return out


class _BorrowedTracer(HipTracer):
    def close(self):
        self.h = None


_api = None


def load_library():
    global _api
    if _api is None:
        _api = HipApi()
    return _api


def scatter_rows(local_image, global_rows, height):
    """Place the packed local rows of one partition into a full-height image."""
    out = np.zeros((height,) + local_image.shape[1:], dtype=local_image.dtype)
    out[global_rows] = local_image
    return out
