#!/usr/bin/env python3
"""Times rt_query_closest_buffers and rt_query_occluded_buffers (include/rt_query.h) on one GPU at 1920 x 1080, next to
rt_render_aov_centre_to_device on the same scene (the yardstick: the same walk for the rays through the pixel centres).

Cases, per scene (configs 2, 3 and 4):
  camera rays through the pixel centres, in 8 x 8 tile order (a wave's 64 rays are one tile, as in the AOV pass) and in row order — closest
      hit, and occlusion with tmax = +inf;
  one hemisphere ray per first hit (origin = the hit position pushed out along the normal, direction = normalize(normal + a random unit
      vector), built in torch from the AOV centre records, in tile order) — closest hit, occlusion with tmax = +inf and with tmax = a tenth
      of the scene's extent (the diagonal of the hit positions' bounds).

HIP events (torch.cuda.Event) on a torch stream given to rt_set_stream around back-to-back enqueued calls; after a warm-up, each figure is
the median of --regions regions (default 9, at least 7) of at least --region-ms (default 60, at least 50) each, with the regions' minimum and
maximum.  torch is imported first, so that the library shares its HIP runtime.  Prints one JSON line; --out FILE also writes a table."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402


def tile_order(w, h):
    """Pixel indices (y * w + x) in the order the AOV pass visits them: 8 x 8 tiles row by row, lane = (y & 7) * 8 + (x & 7)."""
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    key = ((ys // 8) * ((w + 7) // 8) + xs // 8) * 64 + (ys % 8) * 8 + xs % 8
    return torch.from_numpy(np.argsort(key.ravel(), kind="stable"))


def centre_rays(p, w, h, dev):
    """The rays through the unjittered pixel centres from the camera origin (RCC:15, RC:550-558): (h * w, 8) float32 RtRay records."""
    m = torch.tensor(list(p.camLocalToWorld), dtype=torch.float32, device=dev).reshape(4, 4)  # column-major: m[c] is column c
    vp = list(p.viewParams)
    u = torch.arange(w, dtype=torch.float32, device=dev) / (w - 1) - 0.5
    v = torch.arange(h, dtype=torch.float32, device=dev) / (h - 1) - 0.5
    lx, ly = (u * vp[0])[None, :].expand(h, w), (v * vp[1])[:, None].expand(h, w)
    focus = m[0, :3] * lx[..., None] + m[1, :3] * ly[..., None] + m[2, :3] * vp[2] + m[3, :3]
    d = torch.nn.functional.normalize(focus - m[3, :3], dim=-1)
    rays = torch.zeros((h, w, 8), dtype=torch.float32, device=dev)
    rays[..., 0:3] = m[3, :3]
    rays[..., 3] = float("inf")
    rays[..., 4:7] = d
    return rays.reshape(h * w, 8)


def hemisphere_rays(aov, order, tmax, seed):
    """One ray per first hit of the AOV records ((h * w, 16) float32 view), in `order`."""
    rec = aov[order.to(aov.device)]
    rec = rec[(rec[:, 7].view(torch.int32) & 3) != 0]
    n, pos = rec[:, 1:4], rec[:, 4:7]
    g = torch.Generator(device=aov.device).manual_seed(seed)
    r = torch.nn.functional.normalize(torch.randn(n.shape, generator=g, device=aov.device), dim=-1)
    d = torch.nn.functional.normalize(n + 0.999 * r, dim=-1)
    extent = float((pos.max(dim=0).values - pos.min(dim=0).values).norm()) if len(pos) else 1.0
    rays = torch.zeros((len(rec), 8), dtype=torch.float32, device=aov.device)
    rays[:, 0:3] = pos + n * (1e-4 * extent)
    rays[:, 3] = float("inf") if tmax is None else tmax * extent
    rays[:, 4:7] = d
    return rays.contiguous(), extent


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--configs", default="2,3,4")
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--region-ms", type=float, default=60.0)
    ap.add_argument("--out", help="also write the table to this text file")
    a = ap.parse_args()
    if a.regions < 7 or a.region_ms < 50:
        ap.error("at least 7 regions of at least 50 ms")
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    pkg = graft.load_package()
    api = pkg.load_library()
    w, h = a.width, a.height
    stream = torch.cuda.Stream()
    order = tile_order(w, h)

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

    rows = []
    for cfg in [int(c) for c in a.configs.split(",")]:
        tr = api.create_tracer(0)
        mgr = pkg.scenes.get(cfg).make_manager(tr, api, w, h)
        mgr.OnEnable(renderSeed=1)
        tr.synchronize()
        tr.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            aov = torch.zeros((h * w, 16), dtype=torch.float32, device=dev)
            row_rays = centre_rays(mgr.params(), w, h, dev)
            cases = [("centre rays, tile order", row_rays[order.to(dev)].contiguous()), ("centre rays, row order", row_rays)]
            stream.synchronize()
            tr.render_aov_centre_to_device(aov.data_ptr(), aov.numel() * 4)
            tr.synchronize()
            hemi_inf, extent = hemisphere_rays(aov, order, None, 1)
            hemi_short, _ = hemisphere_rays(aov, order, 0.1, 1)
            hits = torch.zeros((h * w, 12), dtype=torch.float32, device=dev)
            occ = torch.zeros((h * w,), dtype=torch.int32, device=dev)
            stream.synchronize()
            t_aov = measure(lambda: tr.render_aov_centre_to_device(aov.data_ptr(), aov.numel() * 4))
            rows.append(dict(config=cfg, case="rt_render_aov_centre_to_device", rays=h * w, **t_aov))
            for what, rays in cases + [("hemisphere rays, tmax = +inf", hemi_inf), ("hemisphere rays, tmax = extent / 10", hemi_short)]:
                n = len(rays)
                if n == 0:
                    continue
                occluded = measure(lambda: tr.query_occluded_buffers(rays.data_ptr(), n, occ.data_ptr()))
                tr.synchronize()
                frac = float(occ[:n].sum().item()) / n
                row = dict(config=cfg, case="occluded: " + what, rays=n, occluded_fraction=frac, **occluded)
                if "extent / 10" not in what:  # (tmax plays no part in the closest hit: one figure per ray set)
                    closest = measure(lambda: tr.query_closest_buffers(rays.data_ptr(), n, hits.data_ptr()))
                    tr.synchronize()
                    c_row = dict(config=cfg, case="closest: " + what, rays=n, **closest)
                    if "tile order" in what:
                        c_row["closest_over_aov_centre"] = closest["median_ms"] / t_aov["median_ms"]
                    rows.append(c_row)
                    row["occluded_over_closest"] = occluded["median_ms"] / closest["median_ms"]
                    last_closest = closest
                else:
                    row["occluded_over_closest"] = occluded["median_ms"] / last_closest["median_ms"]
                rows.append(row)
        tr.set_stream(None)
        tr.synchronize()
        tr.close()
    for r in rows:
        r["Mrays_per_s"] = r["rays"] / r["median_ms"] / 1e3
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    result = {"tool": "query_bench", "width": w, "height": h, "regions": a.regions, "region_ms": a.region_ms, "commit": commit, "rows": rows}
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"rt_query_*_buffers, {w} x {h}; median of {a.regions} regions of >= {a.region_ms:g} ms, [min, max] of the regions; commit {commit}\n\n")
            f.write("config  case                                                    rays     ms per call  [min, max]          Mrays/s   ratio\n")
            for r in rows:
                ratio = r.get("closest_over_aov_centre")
                note = f"{ratio:.3f} closest / AOV centre" if ratio else (f"{r['occluded_over_closest']:.3f} occluded / closest" if "occluded_over_closest" in r else "")
                if "occluded_fraction" in r:
                    note += f" ({100 * r['occluded_fraction']:.1f} % occluded)"
                f.write(f"{r['config']:6d}  {r['case']:54s}  {r['rays']:7d}  {r['median_ms']:11.4f}  [{r['min_ms']:.4f}, {r['max_ms']:.4f}]  {r['Mrays_per_s']:8.1f}   {note}\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
