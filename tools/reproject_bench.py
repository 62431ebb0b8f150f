#!/usr/bin/env python3
"""Times the calls of include/rt_reproject.h and include/rt_motion.h on one GPU: config 3 at 1920 x 1080, a camera move of (0.05, 0.02, 0.03).

HIP events on the stream the context renders on (a stream of this tool's, given to rt_set_stream) around back-to-back enqueued calls;
after a warm-up, each figure is the median of --regions regions (default 9, at least 7) of at least --region-ms (default 60, at least 50)
each, with the regions' minimum and maximum next to it.  Rows:

  rt_reproject_buffers         the pass alone
  rt_resolve_buffers           the per-pixel divide
  rt_reproject_accumulated     AOV pass + copy of the records + reprojection + commit
  rt_render_aov_to_device      the AOV pass alone: the difference to the row above is the call without its AOV pass
  rt_reproject_buffers_moving      the pass with an identity table of the scene's size (three more 16-byte loads per pixel, from cache)
  rt_reproject_accumulated_moving  the context call with that table and the pixel-centre pass (RT_AOV_CENTRE)
  rt_render_aov_centre_to_device   the pixel-centre pass alone
  device copy, reproject       hipMemcpyAsync device to device of the bytes rt_reproject_buffers must move, as the yardstick
  device copy, resolve         the same for rt_resolve_buffers (16 B in + 16 B out per pixel)
  host round trip              what a caller needed before this header: rt_read_accumulated, rt_render_aov, the NumPy restatement
                               (tests/reproject_reference.py, needs the oracle), rt_write_accumulated — wall clock, --host-trips times

Bytes rt_reproject_buffers must move per pixel, before cache reuse: 64 read (the current record) + 16 written + four taps of 16 + 28 read
(the sum; normal, position and object of the record) = 256.  Prints one JSON line; --out FILE also writes the table as text."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

BYTES_REPROJECT = 64 + 16 + 4 * (16 + 28)
BYTES_RESOLVE = 32


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=4, help="frames accumulated before the move")
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--region-ms", type=float, default=60.0)
    ap.add_argument("--host-trips", type=int, default=3, help="repetitions of the host round trip (0: skip it)")
    ap.add_argument("--out", help="also write the table to this text file")
    a = ap.parse_args()
    if a.regions < 7 or a.region_ms < 50:
        ap.error("at least 7 regions of at least 50 ms")
    import numpy as np
    pkg = graft.load_package()
    api = pkg.load_library()
    hip = C.CDLL("libamdhip64.so")

    def ok(rc):
        if rc != 0:
            raise RuntimeError(f"HIP call failed with {rc}")
    w, h = a.width, a.height
    n = w * h
    tr = api.create_tracer(0)
    mgr = pkg.scenes.get(3).make_manager(tr, api, w, h)
    mgr.OnEnable(renderSeed=1)
    mgr.RenderFrames(a.frames)
    tr.synchronize()
    stream = C.c_void_p()
    ok(hip.hipStreamCreate(C.byref(stream)))
    tr.set_stream(stream)
    bufs = {}
    for name, size in (("prev", n * 64), ("cur", n * 64), ("sum", n * 16), ("out", n * 16), ("copy_src", n * BYTES_REPROJECT // 2), ("copy_dst", n * BYTES_REPROJECT // 2)):
        bufs[name] = C.c_void_p()
        ok(hip.hipMalloc(C.byref(bufs[name]), C.c_size_t(size)))
    tr.render_aov_to_device(1, bufs["prev"].value, n * 64)
    models = mgr.meshInfo.copy()
    table = api.motion_table(None, None, models, models)  # nothing moved: an identity table of the scene's size
    n_objects = len(table)
    bufs["motion"] = C.c_void_p()
    ok(hip.hipMalloc(C.byref(bufs["motion"]), C.c_size_t(table.nbytes)))
    ok(hip.hipMemcpy(bufs["motion"], C.c_void_p(table.ctypes.data), C.c_size_t(table.nbytes), C.c_int(1)))
    before = mgr.params()
    t = mgr.camera.transform
    mgr.camera.transform = pkg.Transform(tuple(np.array(t.position) + np.array([0.05, 0.02, 0.03])), t.euler, t.scale)
    mgr.SetShaderParams()
    p = api.reproject_params(before)
    tr.render_aov_to_device(1, bufs["cur"].value, n * 64)
    _, d_acc = tr.render_targets()
    ok(hip.hipMemcpyAsync(bufs["sum"], C.c_void_p(d_acc), C.c_size_t(n * 16), C.c_int(3), stream))
    tr.synchronize()
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        ok(hip.hipEventCreate(C.byref(e)))
    calls = {
        "rt_reproject_buffers": lambda: tr.reproject_buffers(w, h, bufs["sum"].value, bufs["prev"].value, bufs["cur"].value, bufs["out"].value, p),
        "rt_resolve_buffers": lambda: tr.resolve_buffers(w, h, bufs["sum"].value, bufs["out"].value),
        "rt_reproject_accumulated": lambda: tr.reproject_accumulated(p, bufs["prev"].value, 1, bufs["cur"].value),
        "rt_render_aov_to_device": lambda: tr.render_aov_to_device(1, bufs["cur"].value, n * 64),
        "rt_reproject_buffers_moving": lambda: tr.reproject_buffers_moving(w, h, bufs["sum"].value, bufs["prev"].value, bufs["cur"].value, bufs["motion"].value, n_objects,
                                                                           bufs["out"].value, p),
        "rt_reproject_accumulated_moving": lambda: tr.reproject_accumulated_moving(p, bufs["prev"].value, pkg.abi.AOV_CENTRE, bufs["motion"].value, n_objects, bufs["cur"].value),
        "rt_render_aov_centre_to_device": lambda: tr.render_aov_centre_to_device(bufs["cur"].value, n * 64),
        "device copy, reproject": lambda: ok(hip.hipMemcpyAsync(bufs["copy_dst"], bufs["copy_src"], C.c_size_t(n * BYTES_REPROJECT // 2), C.c_int(3), stream)),
        "device copy, resolve": lambda: ok(hip.hipMemcpyAsync(bufs["out"], bufs["sum"], C.c_size_t(n * 16), C.c_int(3), stream)),
    }

    def region(fn, count):
        ok(hip.hipEventRecord(ev[0], stream))
        for _ in range(count):
            fn()
        ok(hip.hipEventRecord(ev[1], stream))
        ok(hip.hipEventSynchronize(ev[1]))
        ms = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]))
        return ms.value / count
    rows = []
    for name, fn in calls.items():
        one = max(min(region(fn, 3), region(fn, 3)), 1e-3)  # warm-up, and the call count a region needs
        count = max(3, int(a.region_ms / one) + 1)
        region(fn, count)
        t_ms = sorted(region(fn, count) for _ in range(a.regions))
        moved = {"rt_reproject_buffers": BYTES_REPROJECT, "rt_reproject_buffers_moving": BYTES_REPROJECT, "device copy, reproject": BYTES_REPROJECT, "rt_resolve_buffers": BYTES_RESOLVE, "device copy, resolve": BYTES_RESOLVE}.get(name)
        rows.append({"call": name, "median_ms": statistics.median(t_ms), "min_ms": t_ms[0], "max_ms": t_ms[-1], "calls_per_region": count,
                     "GB": None if moved is None else moved * n / 1e9, "GB_per_s": None if moved is None else moved * n / 1e6 / statistics.median(t_ms)})
    by = {r["call"]: r for r in rows}
    without_aov = by["rt_reproject_accumulated"]["median_ms"] - by["rt_render_aov_to_device"]["median_ms"]
    tr.synchronize()
    tr.set_stream(None)
    host = None
    if a.host_trips:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import reproject_reference as ref
        orc = graft.load_oracle()
        prev_rec = tr.render_aov(1)
        trips = []
        for _ in range(a.host_trips):
            t0 = time.perf_counter()
            acc, cur_rec = tr.read_accumulated(), tr.render_aov(1)
            tr.write_accumulated(ref.reproject_with(orc, acc, prev_rec, cur_rec, p))
            tr.synchronize()
            trips.append((time.perf_counter() - t0) * 1e3)
        host = {"median_ms": statistics.median(trips), "min_ms": min(trips), "max_ms": max(trips), "trips": a.host_trips}
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    result = {"tool": "reproject_bench", "width": w, "height": h, "frames": a.frames, "regions": a.regions, "region_ms": a.region_ms, "rows": rows,
              "reproject_accumulated_without_aov_pass_ms": without_aov, "host_round_trip": host, "commit": commit}
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"include/rt_reproject.h and include/rt_motion.h, {w} x {h}, config 3 ({a.frames} frames accumulated), camera moved by (0.05, 0.02, 0.03); commit {commit}\n")
            f.write(f"median of {a.regions} regions of >= {a.region_ms:g} ms, [min, max] of the regions\n\n")
            f.write(f"{'call':<32} {'ms per call':>11}   [min, max]            GB moved   GB/s\n")
            for r in rows:
                f.write(f"{r['call']:<32} {r['median_ms']:11.4f}   [{r['min_ms']:.4f}, {r['max_ms']:.4f}]")
                f.write("\n" if r["GB"] is None else f"   {r['GB']:8.3f}   {r['GB_per_s']:5.0f}\n")
            f.write(f"\nrt_reproject_accumulated without its AOV pass (difference of the medians): {without_aov:.4f} ms\n")
            if host:
                f.write(f"host round trip (read, AOV to host, NumPy restatement, write): {host['median_ms']:.0f} ms [{host['min_ms']:.0f}, {host['max_ms']:.0f}], {host['trips']} trips, wall clock\n")
    print(json.dumps(result))
    tr.close()
    for b in bufs.values():
        hip.hipFree(b)


if __name__ == "__main__":
    main()
