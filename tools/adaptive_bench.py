#!/usr/bin/env python3
"""Times the calls of include/rt_adaptive.h on one GPU and compares an adaptive render with a uniform one at equal work.

  select     rt_adaptive_select_buffers at --width x --height (default 1920 x 1080) on synthetic sums and moments: 32 bytes read per
             pixel, stated next to a plain device-to-device copy of the same two images.
  partial    configs 2 and 3 at that size: the time per frame of rt_adaptive_render_frames over lists holding 100, 50, 25, 10 and 2 %
             of the tiles, as one contiguous block and as a scattered set, n = 1 per call and n = 16 fused, next to the time per frame of
             rt_render_frames on the same context (that path does not know about tile lists: it is the figure to compare with).
  quality    config 3 at 320 x 180: the squared error against a --reference-frames (default 4,096) render of a uniform render and of
             the adaptive loop stopped at the same total pixelFrames; the ratio and the histogram of per-pixel frame counts.

Timing: wall clock around calls that only enqueue, closed by rt_synchronize; after a warm-up, each figure is the median of --regions
regions (default 9, at least 7) of at least --region-ms (default 60, at least 50) each, with the regions' minimum and maximum.
Prints one JSON line per section; --out FILE also writes them as text."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402


def regions(run, sync, n_regions, region_ms, unit=1):
    """median / min / max ms per `unit` of run() (which enqueues `unit` units of work), over regions of at least region_ms."""
    for _ in range(3):
        run()
    sync()
    t0 = time.perf_counter()
    run()
    sync()
    one = max((time.perf_counter() - t0) * 1e3, 1e-3)
    reps = max(1, int(np.ceil(region_ms / one)))
    out = []
    for _ in range(n_regions):
        t0 = time.perf_counter()
        for _ in range(reps):
            run()
        sync()
        out.append((time.perf_counter() - t0) * 1e3 / (reps * unit))
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out), "calls_per_region": reps}


def tile_lists(tx, ty, share, rng):
    n = max(1, int(round(tx * ty * share)))
    return {"block": np.arange(n, dtype=np.uint32), "scattered": np.sort(rng.choice(tx * ty, size=n, replace=False)).astype(np.uint32)}


def bench_select(pkg, api, a):
    hip = C.CDLL("libamdhip64.so")
    w, h = a.width, a.height
    tx, ty = (w + 7) // 8, (h + 7) // 8
    rng = np.random.default_rng(1)
    s = np.concatenate([rng.uniform(0, 40, (h, w, 3)), np.full((h, w, 1), 16.0)], axis=-1).astype(np.float32)
    m = np.zeros((h, w, 4), dtype=np.float32)
    mean = rng.uniform(0.05, 2.0, (h, w)).astype(np.float32)
    m[..., 0], m[..., 1], m[..., 3] = mean * 4, mean * mean * (1 + rng.uniform(0, 0.2, (h, w)) ** 2) * 4, 4
    bufs = []

    def dev(nbytes, src=None):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        if src is not None:
            assert hip.hipMemcpy(p, C.c_void_p(src.ctypes.data), C.c_size_t(nbytes), C.c_int(1)) == 0
        bufs.append(p)
        return p
    d_s, d_m, d_copy = dev(s.nbytes, s), dev(m.nbytes, m), dev(s.nbytes + m.nbytes)
    d_te, d_tiles, d_counts = dev(tx * ty * 4), dev(tx * ty * 4), dev(16)
    tr = api.create_tracer(0)
    p = api.adaptive_params()
    sel = regions(lambda: tr.adaptive_select_buffers(w, h, d_s.value, d_m.value, d_te.value, d_tiles.value, d_counts.value, p), tr.synchronize, a.regions, a.region_ms)

    def copy():
        assert hip.hipMemcpyAsync(d_copy, d_s, C.c_size_t(s.nbytes), C.c_int(3), None) == 0
        assert hip.hipMemcpyAsync(C.c_void_p(d_copy.value + s.nbytes), d_m, C.c_size_t(m.nbytes), C.c_int(3), None) == 0
    cp = regions(copy, lambda: hip.hipDeviceSynchronize(), a.regions, a.region_ms)
    counts = np.zeros(4, dtype=np.uint32)
    hip.hipMemcpy(C.c_void_p(counts.ctypes.data), d_counts, C.c_size_t(16), C.c_int(2))
    tr.close()
    for b in bufs:
        hip.hipFree(b)
    mb = (s.nbytes + m.nbytes) / 1e6
    return {"section": "select", "size": [w, h], "tiles": tx * ty, "tiles_active": int(counts[0]), "bytes_read_MB": mb, "select": sel,
            "select_GBps": mb / sel["median_ms"], "device_copy_of_the_same_bytes": cp, "copy_GBps_read": mb / cp["median_ms"]}


def bench_partial(pkg, api, a, cfg):
    w, h = a.width, a.height
    tx, ty = (w + 7) // 8, (h + 7) // 8
    tr = api.create_tracer(0)
    mgr = pkg.scenes.get(cfg).make_manager(tr, api, w, h)
    mgr.OnEnable(renderSeed=1)
    mgr.RenderFrames(64)  # the tile order and the launch tuner settle
    tr.synchronize()
    out = {"section": "partial", "config": cfg, "size": [w, h], "tiles": tx * ty, "rows": []}
    for n in (1, 16):
        full = regions(lambda: tr.render_frames(n), tr.synchronize, a.regions, a.region_ms, unit=n)
        out["rows"].append({"list": "rt_render_frames", "share": 1.0, "n": n, **full})
        rng = np.random.default_rng(7)
        for share in (1.0, 0.5, 0.25, 0.10, 0.02):
            for kind, tiles in tile_lists(tx, ty, share, rng).items():
                if share == 1.0 and kind == "scattered":
                    continue
                tr.adaptive_set_tiles(tiles)
                r = regions(lambda: tr.adaptive_render_frames(n), tr.synchronize, a.regions, a.region_ms, unit=n)
                out["rows"].append({"list": kind, "share": share, "n": n, **r, "of_a_full_frame": r["median_ms"] / full["median_ms"]})
    tr.close()
    return out


def bench_quality(pkg, api, a):
    w, h, cfg = 320, 180, 3

    def tracer():
        tr = api.create_tracer(0)
        mgr = pkg.scenes.get(cfg).make_manager(tr, api, w, h)
        mgr.OnEnable(renderSeed=1)
        return tr, mgr
    tr, mgr = tracer()
    mgr.RenderFrames(a.reference_frames)
    truth = tr.resolve()[..., :3].astype(np.float64)
    tr.close()
    tr, mgr = tracer()
    p = api.adaptive_params(threshold=a.threshold, minFrames=8, maxFrames=a.max_frames)
    for _ in range(2):
        mgr.RenderFrames(4)
        tr.variance_update()
    selections = 0
    while True:
        res = tr.adaptive_select(p)
        selections += 1
        if not res["tiles_active"]:
            break
        tr.adaptive_render_frames(4)
        tr.variance_update()
    work = tr.counters()["pixelFrames"]
    img = tr.resolve()
    count = img[..., 3]
    tr.close()
    uniform_frames = max(1, int(round(work / (w * h))))
    tr, mgr = tracer()
    mgr.RenderFrames(uniform_frames)
    uni = tr.resolve()[..., :3].astype(np.float64)
    tr.close()
    mse_a, mse_u = float(((img[..., :3] - truth) ** 2).mean()), float(((uni - truth) ** 2).mean())
    hist = {str(int(k)): int(v) for k, v in zip(*np.unique(count, return_counts=True))}
    return {"section": "quality", "config": cfg, "size": [w, h], "reference_frames": a.reference_frames, "threshold": a.threshold, "maxFrames": a.max_frames,
            "selections": selections, "adaptive_pixelFrames": int(work), "uniform_frames": uniform_frames, "uniform_pixelFrames": uniform_frames * w * h,
            "mse_adaptive": mse_a, "mse_uniform": mse_u, "mse_adaptive_over_uniform": mse_a / mse_u, "frames_per_pixel_histogram": hist}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--sections", default="select,partial,quality")
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--region-ms", type=float, default=60.0)
    ap.add_argument("--reference-frames", type=int, default=4096)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--max-frames", type=int, default=256)
    ap.add_argument("--out", help="also append the JSON lines to this text file")
    a = ap.parse_args()
    if a.regions < 7 or a.region_ms < 50:
        ap.error("at least 7 regions of at least 50 ms")
    pkg = graft.load_package()
    api = pkg.load_library()
    lines = []
    for sec in a.sections.split(","):
        results = [bench_select(pkg, api, a)] if sec == "select" else [bench_partial(pkg, api, a, c) for c in (2, 3)] if sec == "partial" else [bench_quality(pkg, api, a)]
        for r in results:
            r["tool"] = "adaptive_bench"
            lines.append(json.dumps(r))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
