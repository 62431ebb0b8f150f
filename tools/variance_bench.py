#!/usr/bin/env python3
"""Times the passes of include/rt_variance.h on one GPU next to rt_denoise_buffers: config 3 at 1920 x 1080, 5 iterations, demodulation on.

The method is tools/denoise_bench.py's: HIP events on the stream the context renders on (a stream of this tool's, given to
rt_set_stream) around back-to-back enqueued calls; after a warm-up, each figure is the median of --regions regions (default 9, at least
7) of at least --region-ms (default 60, at least 50) each, with the regions' minimum and maximum next to it.  Timed:
  rt_denoise_buffers and rt_denoise_variance_buffers (the same image, the same records; the moments of 8 one-frame batches),
  rt_moments_update_buffers (48 B read + 32 B written per pixel when a batch is taken, 16 B written otherwise) and its rebase form (16 B + 16 B),
  rt_variance_carry (a reprojection of the moments, its commit, a rebase) with the records of the current view on both sides.
Prints one JSON line; RT_HIP_LIB selects the build, so two builds are compared in one session."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--region-ms", type=float, default=60.0)
    ap.add_argument("--plain-only", action="store_true", help="rt_denoise_buffers alone (a build without rt_variance.h)")
    a = ap.parse_args()
    if a.regions < 7 or a.region_ms < 50:
        ap.error("at least 7 regions of at least 50 ms")
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
    have = not a.plain_only
    for _ in range(8):
        mgr.RenderFrames(1)
        if have:
            tr.variance_update()
    tr.synchronize()
    stream = C.c_void_p()
    ok(hip.hipStreamCreate(C.byref(stream)))
    tr.set_stream(stream)

    def dev(nbytes):
        p = C.c_void_p()
        ok(hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)))
        ok(hip.hipMemset(p, 0, C.c_size_t(nbytes)))
        return p.value
    d_aov, d_out, d_mean, d_m, d_snap = dev(n * 64), dev(n * 16), dev(n * 16), dev(n * 16), dev(n * 16)
    tr.render_aov_to_device(1, d_aov, n * 64)
    tr.resolve_to_device(d_mean, n * 16)
    if have:
        tr.moments_to_device(d_m, n * 16)
    tr.synchronize()
    _, d_acc = tr.render_targets()
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        ok(hip.hipEventCreate(C.byref(e)))

    def region(fn, calls):
        ok(hip.hipEventRecord(ev[0], stream))
        for _ in range(calls):
            fn()
        ok(hip.hipEventRecord(ev[1], stream))
        ok(hip.hipEventSynchronize(ev[1]))
        ms = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]))
        return ms.value / calls

    def measure(fn):
        one = max(min(region(fn, 3), region(fn, 3)), 1e-3)  # warm-up, and the call count a region needs
        calls = max(3, int(a.region_ms / one) + 1)
        region(fn, calls)
        t = sorted(region(fn, calls) for _ in range(a.regions))
        return {"median_ms": statistics.median(t), "min_ms": t[0], "max_ms": t[-1], "calls_per_region": calls}
    plain = api.denoise_params(iterations=a.iterations, demodulate=1, scale=1.0)
    out = {"tool": "variance_bench", "lib": os.environ.get("RT_HIP_LIB") or "default", "width": w, "height": h, "iterations": a.iterations,
           "regions": a.regions, "region_ms": a.region_ms}
    out["rt_denoise_buffers"] = measure(lambda: tr.denoise_buffers(w, h, d_mean, d_aov, d_out, plain))
    if have:
        p = api.variance_denoise_params(iterations=a.iterations, demodulate=1)
        out["rt_denoise_variance_buffers"] = measure(lambda: tr.denoise_variance_buffers(w, h, d_mean, d_m, d_aov, d_out, p))
        for k in range(1, a.iterations + 1):
            q = api.variance_denoise_params(iterations=k, demodulate=1)
            pk = api.denoise_params(iterations=k, demodulate=1, scale=1.0)
            out[f"variance_{k}_iterations"] = measure(lambda: tr.denoise_variance_buffers(w, h, d_mean, d_m, d_aov, d_out, q))
            out[f"plain_{k}_iterations"] = measure(lambda: tr.denoise_buffers(w, h, d_mean, d_aov, d_out, pk))
        # the snapshot follows the sum, so a second update of the same sum sees no growth: alternate the sum with an empty one — every
        # other call takes a batch (48 B read, 32 B written per pixel), the one between only moves the snapshot (48 B, 16 B): 72 B on average
        d_zero = dev(n * 16)
        turn = [0]

        def update():
            turn[0] ^= 1
            tr.moments_update_buffers(w, h, d_acc if turn[0] else d_zero, d_snap, d_out)
        up = measure(update)
        up["bytes_per_pixel"] = 72
        up["GB_per_s"] = n * 72 / 1e6 / up["median_ms"]
        out["rt_moments_update_buffers"] = up
        rb = measure(lambda: tr.moments_update_buffers(w, h, d_acc, d_snap, d_out, rebase=True))
        rb["GB_per_s"] = n * 32 / 1e6 / rb["median_ms"]
        out["rt_moments_update_buffers_rebase"] = rb
        rp = api.reproject_params(mgr.params())
        out["rt_variance_carry"] = measure(lambda: tr.variance_carry(rp, d_aov, d_aov))
    print(json.dumps(out))
    tr.synchronize()
    tr.set_stream(None)
    tr.close()
    for d in (d_aov, d_out, d_mean, d_m, d_snap):
        hip.hipFree(C.c_void_p(d))


if __name__ == "__main__":
    main()
