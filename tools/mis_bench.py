#!/usr/bin/env python3
"""Time per path and equal-time efficiency of rt_mis_trace's device form (include/rt_mis.h) against rt_nee_trace_buffers and
rt_radiance_trace_buffers of the same build, on one GPU.  tools/nee_bench.py's method and batch: the 320 x 180 pixel-centre camera rays
of a config (tools/radiance_bench.py's rays, in 8 x 8 tile order), and for each of the three passes

  variance     the per-sample variance of luminance: every pixel's unbiased sample variance over --samples chained samples, averaged
               over the pixels, in float64 on the device; with the image's mean luminance next to it (plain and mis have the same
               expectation at every maxBounceCount; nee carries one bounce more of emitter light);
  ms / Mpaths  device time per million paths: HIP events on a torch stream given to rt_set_stream around back-to-back enqueued calls;
               after a warm-up (which also lets the clock ramp: the first regions of a cold device run slower), the median of --regions
               regions (default 9, at least 7) of at least --region-ms (default 60, at least 50) each, with their minimum and maximum;
  product      variance x ms / Mpaths; the ratio of two passes' products is the equal-time efficiency of one over the other.

Variance and efficiency are reported for --configs (default 1,3), time alone also for --time-configs (default 4).  No ratio is required
of it.  torch is imported first, so that the library shares its HIP runtime.  Prints one JSON line; --out FILE also writes a table."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as graft  # noqa: E402
from radiance_bench import centre_path_rays, tile_order  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--height", type=int, default=180)
    ap.add_argument("--configs", default="1,3", help="variance, time and efficiency")
    ap.add_argument("--time-configs", default="4", help="time only")
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--region-ms", type=float, default=60.0)
    ap.add_argument("--out", help="also write the table to this text file")
    a = ap.parse_args()
    if a.regions < 7 or a.region_ms < 50 or a.samples < 2:
        ap.error("at least 7 regions of at least 50 ms, and at least 2 samples")
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    pkg = graft.load_package()
    api = pkg.load_library()
    w, h = a.width, a.height
    n = w * h
    stream = torch.cuda.Stream()
    order = tile_order(w, h).to(dev)
    lum = torch.tensor([0.2126, 0.7152, 0.0722], dtype=torch.float64, device=dev)

    def measure(call):
        def region(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(calls):
                call()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / calls
        one = max(min(region(3), region(3)), 1e-3)  # warm-up, and the call count a region needs
        calls = max(3, int(a.region_ms / one) + 1)
        region(calls)
        t = sorted(region(calls) for _ in range(a.regions))
        return {"median_ms": statistics.median(t), "min_ms": t[0], "max_ms": t[-1], "calls_per_region": calls}

    full = [int(c) for c in a.configs.split(",") if c]
    timed = [int(c) for c in a.time_configs.split(",") if c]
    rows = []
    for cfg in full + [c for c in timed if c not in full]:
        tr = api.create_tracer(0)
        mgr = pkg.scenes.get(cfg).make_manager(tr, api, w, h)
        mgr.numRaysPerPixel, mgr.defocusStrength, mgr.divergeStrength = 1, 0.0, 0.0
        mgr.InitBVH()
        mgr.SetShaderParams()
        lights = tr.nee_light_count()
        tr.synchronize()
        tr.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            first = centre_path_rays(mgr.params(), w, h, dev)[order].contiguous()
            out = torch.zeros((n, 4), dtype=torch.int32, device=dev)
            stream.synchronize()
            for what, call in (("plain", tr.radiance_trace_buffers), ("nee", tr.radiance_trace_nee_buffers), ("mis", tr.radiance_trace_mis_buffers)):
                mean_lum = variance = largest = None
                if cfg in full:
                    rays = first.clone()
                    s1 = torch.zeros(n, dtype=torch.float64, device=dev)
                    s2 = torch.zeros(n, dtype=torch.float64, device=dev)
                    top = torch.zeros((), dtype=torch.float64, device=dev)
                    for _ in range(a.samples):
                        call(rays.data_ptr(), n, out.data_ptr())
                        y = out[:, :3].view(torch.float32).to(torch.float64) @ lum
                        s1 += y
                        s2 += y * y
                        top = torch.maximum(top, y.max())
                        rays[:, 7] = out[:, 3]  # chain: the state this sample left starts the next one
                    tr.synchronize()
                    mean = s1 / a.samples
                    var = (s2 - a.samples * mean * mean) / (a.samples - 1)
                    mean_lum, variance, largest = float(mean.mean()), float(var.mean()), float(top)
                t = measure(lambda: call(first.data_ptr(), n, out.data_ptr()))
                tr.synchronize()
                ms_per_mpaths = t["median_ms"] * 1e6 / n
                rows.append(dict(config=cfg, case=what, rays=n, samples=a.samples if cfg in full else 0, maxBounceCount=int(mgr.maxBounceCount), sphere_entries=lights[0],
                                 triangle_entries=lights[1], mean_luminance=mean_lum, variance=variance, largest_sample=largest, ms_per_mpaths=ms_per_mpaths,
                                 product=None if variance is None else variance * ms_per_mpaths, **t))
        tr.set_stream(None)
        tr.synchronize()
        tr.close()
    by = {(r["config"], r["case"]): r for r in rows}
    for r in rows:
        if r["case"] == "plain":
            continue
        for other in ("plain", "nee"):
            o = by[(r["config"], other)]
            if o is r:
                continue
            r[f"time_ratio_over_{other}"] = r["ms_per_mpaths"] / o["ms_per_mpaths"]
            if r["product"]:
                r[f"variance_ratio_{other}_over_this"] = o["variance"] / r["variance"]
                r[f"equal_time_efficiency_over_{other}"] = o["product"] / r["product"]
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    result = {"tool": "mis_bench", "width": w, "height": h, "samples": a.samples, "regions": a.regions, "region_ms": a.region_ms, "commit": commit, "rows": rows}
    if a.out:
        def num(v, spec):
            return format(v, spec) if v is not None else "-".rjust(len(format(0.0, spec)))
        with open(a.out, "w") as f:
            f.write(f"mis_bench, {w} x {h} pixel-centre camera rays in tile order, {a.samples} chained samples per pixel; time: median of {a.regions} regions of >= {a.region_ms:g} ms "
                    "behind a warm-up region, [min, max] of the regions\n\n")
            f.write("config  bounces  lights (sph, tri)  case   mean lum   variance      largest     ms per call  [min, max]          ms / Mpaths   variance x ms/Mpaths\n")
            for r in rows:
                f.write(f"{r['config']:6d}  {r['maxBounceCount']:7d}  {r['sphere_entries']:7d} {r['triangle_entries']:7d}    {r['case']:5s}  {num(r['mean_luminance'], '8.5f')}  "
                        f"{num(r['variance'], '12.6e')}  {num(r['largest_sample'], '10.3f')}  {r['median_ms']:10.4f}  [{r['min_ms']:.4f}, {r['max_ms']:.4f}]  {r['ms_per_mpaths']:10.3f}   "
                        f"{num(r['product'], '12.6e')}\n")
            f.write("\n")
            for r in rows:
                for other in ("plain", "nee"):
                    if f"time_ratio_over_{other}" not in r:
                        continue
                    line = f"config {r['config']}: {r['case']} against {other}: time {r['case']} / {other} = {r[f'time_ratio_over_{other}']:.3f}"
                    if f"equal_time_efficiency_over_{other}" in r:
                        line += (f", variance {other} / {r['case']} = {r[f'variance_ratio_{other}_over_this']:.4g}, "
                                 f"equal-time efficiency of {r['case']} over {other} = {r[f'equal_time_efficiency_over_{other}']:.4g}")
                    f.write(line + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
