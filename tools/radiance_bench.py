#!/usr/bin/env python3
"""Times rt_radiance_trace_buffers (include/rt_radiance.h) on one GPU for the 1920 x 1080 pixel-centre rays of configs 2, 3 and 4, next
to rt_render_frames(1) on the same scene with numRaysPerPixel = 1, defocus and diverge 0 and the same maxBounceCount: the same kind of
paths through the tuned frame kernels (the yardstick).

Cases, per scene:
  frame     rt_render_frames(1), accumulating, one frame per call (`--cases frame`; with `--lib FILE` the library of another build, e.g.
            the parent commit's: the tool then runs that library's frame and nothing else);
  radiance  the camera rays through the unjittered pixel centres, each with a generator state hashed from its pixel index, built in
            torch: in 8 x 8 tile order (a wave's block of 64 rays is one tile, as in the frame kernel), in row order, and shuffled.

`--frame-json FILE` takes the frame times from the JSON line an earlier run printed (so that the two libraries are timed in processes of
their own) and adds the ratio radiance / frame per config.  RT_SUSPEND=N (1 ... 7) in the environment pins the suspension threshold of
the traversal to N/8, for the radiance pass as for the frame kernels (scheduling only).

HIP events (torch.cuda.Event) on a torch stream given to rt_set_stream around back-to-back enqueued calls; after a warm-up, each figure is
the median of --regions regions (default 9, at least 7) of at least --region-ms (default 60, at least 50) each, with the regions' minimum
and maximum.  torch is imported first, so that the library shares its HIP runtime.  Prints one JSON line; --out FILE also writes a table."""
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
    """Pixel indices (y * w + x) in the order the frame kernel hands them out: 8 x 8 tiles row by row, slot = (y & 7) * 8 + (x & 7)."""
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    key = ((ys // 8) * ((w + 7) // 8) + xs // 8) * 64 + (ys % 8) * 8 + xs % 8
    return torch.from_numpy(np.argsort(key.ravel(), kind="stable"))


def centre_path_rays(p, w, h, dev):
    """RtPathRay records ((h * w, 8) int32 view) of the rays through the unjittered pixel centres from the camera origin (RCC:15,
    RC:550-558), rng = a hash of the pixel index (any state gives a path of the frame's kind; the frame's own states are not restated)."""
    m = torch.tensor(list(p.camLocalToWorld), dtype=torch.float32, device=dev).reshape(4, 4)  # column-major: m[c] is column c
    vp = list(p.viewParams)
    u = torch.arange(w, dtype=torch.float32, device=dev) / (w - 1) - 0.5
    v = torch.arange(h, dtype=torch.float32, device=dev) / (h - 1) - 0.5
    lx, ly = (u * vp[0])[None, :].expand(h, w), (v * vp[1])[:, None].expand(h, w)
    focus = m[0, :3] * lx[..., None] + m[1, :3] * ly[..., None] + m[2, :3] * vp[2] + m[3, :3]
    d = torch.nn.functional.normalize(focus - m[3, :3], dim=-1)
    rays = torch.zeros((h, w, 8), dtype=torch.float32, device=dev)
    rays[..., 0:3] = m[3, :3]
    rays[..., 4:7] = d
    rays = rays.reshape(h * w, 8).view(torch.int32)
    idx = torch.arange(h * w, dtype=torch.int64, device=dev)
    state = ((idx * 747796405 + 2891336453) ^ (idx >> 7) * 277803737) & 0xffffffff
    rays[:, 7] = torch.where(state >= 1 << 31, state - (1 << 32), state).to(torch.int32)
    return rays.contiguous()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--configs", default="2,3,4")
    ap.add_argument("--cases", default="frame,radiance", help="comma list of: frame, radiance")
    ap.add_argument("--lib", help="load this libraytrace_hip.so instead of the tree's (frame case only)")
    ap.add_argument("--frame-json", help="take the frame times from the JSON line of an earlier run in this file")
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--region-ms", type=float, default=60.0)
    ap.add_argument("--out", help="also write the table to this text file")
    a = ap.parse_args()
    if a.regions < 7 or a.region_ms < 50:
        ap.error("at least 7 regions of at least 50 ms")
    cases = a.cases.split(",")
    if a.lib and cases != ["frame"]:
        ap.error("--lib times another build's frame: use it with --cases frame")
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    pkg = graft.load_package()
    class OtherBuild(pkg.hip.HipApi):
        """A library of another commit: calls it does not export yet stay unbound (the frame case uses none of them)."""

        def _bind(self, name, res, args):
            if self.has(name):
                super()._bind(name, res, args)

    api = OtherBuild(a.lib) if a.lib else pkg.load_library()
    w, h = a.width, a.height
    stream = torch.cuda.Stream()
    order = tile_order(w, h)
    frame_ms = {}
    if a.frame_json:
        for line in open(a.frame_json):
            if line.startswith("{"):
                for r in json.loads(line)["rows"]:
                    if r["case"] == "frame":
                        frame_ms[r["config"]] = (r["median_ms"], r.get("library"))

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
        mgr.numRaysPerPixel, mgr.defocusStrength, mgr.divergeStrength = 1, 0.0, 0.0
        mgr.OnEnable(renderSeed=1)
        tr.synchronize()
        tr.set_stream(stream.cuda_stream)
        common = dict(config=cfg, rays=h * w, maxBounceCount=int(mgr.maxBounceCount))
        with torch.cuda.stream(stream):
            if "frame" in cases:
                t = measure(lambda: tr.render_frames(1))
                tr.synchronize()
                rows.append(dict(common, case="frame", library=os.path.abspath(a.lib) if a.lib else "this tree", **t))
                frame_ms[cfg] = (t["median_ms"], rows[-1]["library"])
            if "radiance" in cases:
                row_rays = centre_path_rays(mgr.params(), w, h, dev)
                g = torch.Generator().manual_seed(1)
                sets = [("tile order", row_rays[order.to(dev)].contiguous()), ("row order", row_rays),
                        ("shuffled", row_rays[torch.randperm(h * w, generator=g).to(dev)].contiguous())]
                out = torch.zeros((h * w, 4), dtype=torch.int32, device=dev)
                stream.synchronize()
                for what, rays in sets:
                    t = measure(lambda: tr.radiance_trace_buffers(rays.data_ptr(), h * w, out.data_ptr()))
                    tr.synchronize()
                    row = dict(common, case="radiance: centre rays, " + what, suspend=os.environ.get("RT_SUSPEND", "default"),
                               mean_rgb=[float(x) for x in out[:, :3].view(torch.float32).mean(dim=0)], **t)
                    if what == "tile order" and cfg in frame_ms:
                        row["radiance_over_frame"] = t["median_ms"] / frame_ms[cfg][0]
                        row["frame_library"] = frame_ms[cfg][1]
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
    result = {"tool": "radiance_bench", "width": w, "height": h, "regions": a.regions, "region_ms": a.region_ms, "commit": commit, "rows": rows}
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"radiance_bench, {w} x {h}; median of {a.regions} regions of >= {a.region_ms:g} ms, [min, max] of the regions; RT_SUSPEND={os.environ.get('RT_SUSPEND', 'unset')}\n\n")
            f.write("config  bounces  case                                    rays     ms per call  [min, max]            Mrays/s   ratio\n")
            for r in rows:
                note = f"{r['radiance_over_frame']:.3f} radiance / frame" if "radiance_over_frame" in r else ""
                f.write(f"{r['config']:6d}  {r['maxBounceCount']:7d}  {r['case']:38s}  {r['rays']:7d}  {r['median_ms']:11.4f}  [{r['min_ms']:.4f}, {r['max_ms']:.4f}]  {r['Mrays_per_s']:8.1f}   {note}\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
