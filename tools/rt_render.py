#!/usr/bin/env python
"""Render a scene (BASELINE config id or a JSON scene file, see ray_tracing_amd/sceneio.py) on the GPU:

    python tools/rt_render.py 3 --frames 8 --png out.png
    python tools/rt_render.py scene.json --size 960x540 --frames 32 --png out.png --pfm out.pfm --checkpoint ck.npz
    python tools/rt_render.py scene.json --resume ck.npz --frames 32 --png more.png
    python tools/rt_render.py "Assets/Scenes/Glass Balls.unity" --stand-in Icosphere.obj=icosphere:4 --dump-json balls.json
    python tools/rt_render.py 3 --frames 1 --cost-png cost.png --cost-field boxTests --cost-scale 200

--cost-png writes a heatmap of the work the rays of one frame (--cost-frame, default 1) do per pixel (rt_render_cost,
include/rt_cost.h): --cost-field is a column of RtPixelCost or boxTests (= 2 x innerSteps, RC:271); a pixel is grey
value / --cost-scale, or pure red above the scale.
    python tools/rt_render.py 3 --frames 1 --aov-png aov --aov-npy aov.npy

--aov-png PREFIX writes PREFIX_normal.png, PREFIX_albedo.png, PREFIX_depth.png and PREFIX_object.png: what camera ray 0 of
frame --aov-frame (default 1) hits first in every pixel (rt_render_aov, include/rt_aov.h); --aov-npy FILE saves the raw
records (numpy, abi.AOV_DTYPE, rows bottom-up).
    python tools/rt_render.py 3 --frames 4 --png noisy.png --denoise-png denoised.png

--denoise-png FILE writes the accumulated image through the edge-avoiding a-trous filter (rt_denoise, include/rt_denoise.h) with
scale = 1 / frames accumulated, guided by the AOV pass of frame --aov-frame, as an sRGB picture (display.linear_srgb8);
--denoise-iterations N (0..8) and --denoise-sigma COLOUR,NORMAL,PLANE override the library's default parameters.
    python tools/rt_render.py 3 --frames 32 --reproject-png moved --reproject-move 0.05,0.02,0.03 --reproject-frames 4

--reproject-png PREFIX: after the --frames frames, moves the camera by --reproject-move DX,DY,DZ (world units), carries the accumulated
image into the new view (rt_reproject_accumulated, include/rt_reproject.h), renders --reproject-frames more frames and writes
PREFIX_resolved.png (rt_resolve: every pixel divided by its own frame count) and PREFIX_history.png (that count, white =
--frames + --reproject-frames, black = restarted); --reproject-centre steers it by the records of the unjittered pixel centres
(rt_reproject_accumulated_moving with RT_AOV_CENTRE, include/rt_motion.h).  It runs last: the other outputs show the view before the move.

    python tools/rt_render.py 3 --frames 8 --png noisy.png --vdenoise-png filtered.png --variance-png sd.png

--vdenoise-png FILE renders the --frames frames in --variance-batches equal batches (default 8), takes a batch of luminance moments after
each (rt_variance_update, include/rt_variance.h) and writes the accumulated image through the variance-guided a-trous filter
(rt_denoise_variance; --denoise-iterations applies to it too).  --variance-png FILE writes the standard deviation of the mean those
moments give, as a heatmap: grey = sd / --variance-scale (default 0.25), pure red above the scale, blue where fewer than two batches
are known.

    python tools/rt_render.py 3 --frames 64 --adaptive 0.05 --png adaptive.png --adaptive-png counts.png

--adaptive THRESHOLD spends the --frames frames (as a budget of frames x pixels) where the image is noisy (include/rt_adaptive.h): two
full batches of --adaptive-batch frames (default 4) with a batch of luminance moments after each (rt_variance_update), then
rt_adaptive_select — the 8 x 8 tiles whose relative standard error of the mean luminance exceeds THRESHOLD, with --adaptive-min /
--adaptive-max frames per pixel (default: the library's) — and rt_adaptive_render_frames of the next batch on those tiles alone, until no
tile is active or the budget is spent.  --png / --pfm then hold the per-pixel resolve (rt_resolve: every pixel divided by its own frame
count), and --adaptive-png FILE writes that count, white = the largest.

    python tools/rt_render.py 3 --frames 1 --ao-png ao.png --ao-samples 32

--ao-png FILE writes an ambient-occlusion picture made on the device with the ray queries of include/rt_query.h: the records of the
pixel centres (rt_render_aov_centre_to_device) stay in a torch tensor, torch builds --ao-samples (default 16) cosine-weighted hemisphere
rays per first hit (origin = the hit position pushed out along the normal, tmax = --ao-distance of the hits' extent, default 0.25),
rt_query_occluded_buffers answers each batch into a tensor, and the picture is 1 - the mean answer (misses white).  Needs torch, which
is then imported before the library is loaded so that both share one HIP runtime.

    python tools/rt_render.py 3 --frames 1 --panorama-png pano.png --panorama-samples 64

--panorama-png FILE writes an equirectangular 360 x 180 degree view from the camera position, made with the path tracer of
include/rt_radiance.h on rays the camera of the library does not have: torch builds one ray per texel of a --panorama-size image
(default 1024x512; longitude along x, latitude along y, jittered inside the texel) with a generator state per texel,
rt_radiance_trace_buffers traces them into a tensor, and each of the --panorama-samples samples (default 16) starts from the state the
previous one returned (the chain of RtRadiance.rng).  The picture is the mean.  Needs torch, imported before the library.

A Unity scene file is converted by ray_tracing_amd/unityscene.py; meshes that only exist inside the
engine or are missing on disk need `--stand-in NAME=SPEC` (SPEC: cube | quad | rounded_cube |
icosphere:SUBDIV[:DISPLACEMENT_SEED[:RADIUS]] | a JSON mesh spec); a stand-in has to have the
asset's native size, the scene only stores the Transform on top of it.
"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("--frames", type=int, default=None)
    ap.add_argument("--size", default=None, help="WxH override")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--png"); ap.add_argument("--pfm"); ap.add_argument("--checkpoint"); ap.add_argument("--resume")
    ap.add_argument("--dump-json", help="write the scene as JSON and exit (no GPU needed)")
    ap.add_argument("--assets", help="Unity Assets directory (for .unity scenes; default: the scene's project)")
    ap.add_argument("--stand-in", action="append", default=[], metavar="NAME=SPEC", help="mesh stand-in for a .unity scene")
    ap.add_argument("--cost-png", help="heatmap of the per-pixel traversal cost of one frame (rt_render_cost)")
    ap.add_argument("--cost-field", default="boxTests", help="RtPixelCost column, or boxTests = 2 x innerSteps (default)")
    ap.add_argument("--cost-scale", type=float, help="value drawn white; above it a pixel is red (required with --cost-png)")
    ap.add_argument("--cost-frame", type=int, default=1, help="frame (Frame uniform, >= 1) whose rays are counted (default 1)")
    ap.add_argument("--aov-png", metavar="PREFIX", help="first-hit feature buffers of one frame as PREFIX_{normal,albedo,depth,object}.png (rt_render_aov)")
    ap.add_argument("--aov-npy", metavar="FILE", help="the raw RtPixelAov records of that frame as a numpy file")
    ap.add_argument("--aov-frame", type=int, default=1, help="frame (Frame uniform, >= 1) whose camera rays are reported (default 1)")
    ap.add_argument("--denoise-png", metavar="FILE", help="the accumulated image through rt_denoise, as an sRGB picture")
    ap.add_argument("--denoise-iterations", type=int, help="passes of the filter, 0..8 (default: the library's)")
    ap.add_argument("--denoise-sigma", metavar="C,N,P", help="sigmaColour,sigmaNormal,sigmaPlane (default: the library's)")
    ap.add_argument("--vdenoise-png", metavar="FILE", help="the accumulated image through rt_denoise_variance, as an sRGB picture")
    ap.add_argument("--variance-png", metavar="FILE", help="heatmap of the standard deviation of the mean (from the luminance moments)")
    ap.add_argument("--variance-batches", type=int, default=8, help="equal batches the frames are rendered in for the moments (default 8)")
    ap.add_argument("--variance-scale", type=float, default=0.25, help="standard deviation drawn white; above it a pixel is red")
    ap.add_argument("--adaptive", type=float, metavar="THRESHOLD", help="render further frames only on tiles whose relative standard error exceeds THRESHOLD (rt_adaptive_*)")
    ap.add_argument("--adaptive-min", type=int, help="frames every pixel gets at least (default: the library's)")
    ap.add_argument("--adaptive-max", type=int, help="frames after which a pixel no longer keeps its tile active, 0 = no cap (default: the library's)")
    ap.add_argument("--adaptive-batch", type=int, default=4, help="frames between two selections = frames of one batch of moments (default 4)")
    ap.add_argument("--adaptive-png", metavar="FILE", help="the per-pixel frame count after --adaptive, white = the largest")
    ap.add_argument("--reproject-png", metavar="PREFIX", help="move the camera, reproject, render on; PREFIX_resolved.png and PREFIX_history.png")
    ap.add_argument("--reproject-move", metavar="DX,DY,DZ", default="0.05,0.02,0.03", help="camera offset in world units")
    ap.add_argument("--reproject-frames", type=int, default=4, help="frames rendered after the reprojection")
    ap.add_argument("--reproject-centre", action="store_true", help="steer --reproject-png by pixel-centre records (include/rt_motion.h) instead of those of --aov-frame")
    ap.add_argument("--ao-png", metavar="FILE", help="ambient occlusion from rt_query_occluded_buffers on torch-generated hemisphere rays")
    ap.add_argument("--ao-samples", type=int, default=16, help="hemisphere rays per first hit (default 16)")
    ap.add_argument("--ao-distance", type=float, default=0.25, help="tmax of the rays as a fraction of the hits' extent (default 0.25)")
    ap.add_argument("--panorama-png", metavar="FILE", help="equirectangular 360 x 180 view from the camera position through rt_radiance_trace_buffers")
    ap.add_argument("--panorama-samples", type=int, default=16, help="paths per texel, chained through the returned generator state (default 16)")
    ap.add_argument("--panorama-size", default="1024x512", help="WxH of the panorama (default 1024x512)")
    a = ap.parse_args()
    if a.cost_png and a.cost_scale is None:
        ap.error("--cost-png needs --cost-scale")
    if a.panorama_png:
        try:
            pano_w, pano_h = (int(v) for v in a.panorama_size.lower().split("x"))
        except ValueError:
            ap.error("--panorama-size is WxH")
        if a.panorama_samples < 1 or pano_w < 1 or pano_h < 1 or pano_w * pano_h > 1 << 26:
            ap.error("--panorama-samples must be >= 1 and --panorama-size at most 2^26 texels")
        import torch  # before the library: one HIP runtime for both
        torch.cuda.set_device(0)
    if a.ao_png:
        if a.ao_samples < 1 or not a.ao_distance > 0:
            ap.error("--ao-samples must be >= 1 and --ao-distance > 0")
        import torch  # before the library: one HIP runtime for both
        torch.cuda.set_device(0)
    pkg = g.load_package()

    def mesh_spec(text):
        if text.startswith("{"):
            return json.loads(text)
        parts = text.split(":")
        spec = {"type": parts[0]}
        if parts[0] == "icosphere":
            spec["subdivisions"] = int(parts[1]) if len(parts) > 1 else 3
            if len(parts) > 2 and parts[2]:
                spec["displacement_seed"] = int(parts[2])
            if len(parts) > 3:
                spec["radius"] = float(parts[3])   # the stand-in must have the asset's native size
        return spec
    if a.scene.isdigit():
        scene = pkg.scenes.get(int(a.scene))
    elif a.scene.lower().endswith(".unity"):
        stand = dict((kv.split("=", 1)[0], mesh_spec(kv.split("=", 1)[1])) for kv in a.stand_in)
        scene = pkg.sceneio.load_scene(a.scene, assets_dir=a.assets, stand_ins=stand)
    else:
        scene = pkg.sceneio.load_scene(a.scene)
    if a.dump_json:
        pkg.sceneio.save_scene(a.dump_json, scene)
        return
    w, h = (int(x) for x in a.size.split("x")) if a.size else (scene.width, scene.height)
    api = pkg.load_library()
    tr = api.create_tracer(0)
    mgr = scene.make_manager(tr, api, w, h)
    if a.resume:
        meta = pkg.display.load_checkpoint(a.resume, mgr)
        print("resumed at frame", meta["numAccumulatedFrames"])
    else:
        mgr.OnEnable(renderSeed=a.seed)
    frames = a.frames if a.frames is not None else scene.frames
    variance = bool(a.vdenoise_png or a.variance_png)
    if variance and (a.variance_batches < 2 or frames % a.variance_batches):
        ap.error(f"--variance-batches must be at least 2 and divide --frames ({frames})")
    adaptive = None
    if a.adaptive is not None:
        if variance or a.resume or a.adaptive_batch < 1 or frames < 2 * a.adaptive_batch:
            ap.error("--adaptive needs --frames >= 2 x --adaptive-batch and goes with neither --resume nor the --variance outputs")
        fields = {k: v for k, v in (("minFrames", a.adaptive_min), ("maxFrames", a.adaptive_max)) if v is not None}
        adaptive = api.adaptive_params(threshold=a.adaptive, **fields)
    elif a.adaptive_png:
        ap.error("--adaptive-png needs --adaptive")
    tr.reset_counters(); tr.timer_begin()
    if adaptive is not None:
        batch, budget, rounds, active = a.adaptive_batch, frames * w * h, 0, None
        for _ in range(2):
            mgr.RenderFrames(batch)
            tr.variance_update()
        spent = 2 * batch * w * h
        while True:
            active = tr.adaptive_select(adaptive)
            if active["tiles_active"] == 0 or spent + active["pixels_active"] * batch > budget:
                break
            tr.adaptive_render_frames(batch)
            tr.variance_update()
            spent += active["pixels_active"] * batch
            rounds += 1
        mgr.numAccumulatedFrames = tr.frame()  # the manager did not see the adaptive frames
    elif variance:
        tr.variance_reset()  # (a resumed sum is where the batches start from)
        for _ in range(a.variance_batches):
            mgr.RenderFrames(frames // a.variance_batches)
            tr.variance_update()
    else:
        mgr.RenderFrames(frames)
    tr.timer_end(); c = tr.counters()
    print(json.dumps({"scene": scene.name, "size": [w, h], "frames": frames, "spp_total": (mgr.numAccumulatedFrames - 1) * mgr.numRaysPerPixel,
                      "gpu_ms": c["gpuMs"], "Mrays_per_s": c["segments"] / max(c["gpuMs"], 1e-9) / 1e3}))
    disp = pkg.display.RayTraceDisplay(mgr)
    if adaptive is not None:  # pixels hold different numbers of frames: the per-pixel resolve, not Display.shader's division by Frame
        import numpy as np
        img = tr.resolve()
        count = img[..., 3]
        if a.png: pkg.display.write_png(a.png, pkg.display.linear_srgb8(img))
        if a.pfm: pkg.display.write_pfm(a.pfm, img[..., :3])
        if a.adaptive_png:
            grey = np.repeat((count / max(float(count.max()), 1.0))[..., None], 3, axis=-1).astype(np.float32)
            pkg.display.write_png(a.adaptive_png, pkg.display.linear_srgb8(grey))
        print(json.dumps({"adaptive": a.adaptive, "minFrames": adaptive.minFrames, "maxFrames": adaptive.maxFrames, "batch": a.adaptive_batch, "selections": rounds + 1,
                          "tiles_active_at_the_end": active["tiles_active"], "pixel_frames": int(c["pixelFrames"]), "budget": frames * w * h,
                          "frames_per_pixel": {"min": float(count.min()), "mean": float(count.mean()), "max": float(count.max())}}))
    else:
        if a.png: disp.save_png(a.png)
        if a.pfm: disp.save_pfm(a.pfm)
    if a.checkpoint: pkg.display.save_checkpoint(a.checkpoint, mgr)
    if a.cost_png:
        cost = tr.render_cost(a.cost_frame)
        heat = pkg.display.cost_heatmap_srgb8(cost, a.cost_field, a.cost_scale)
        pkg.display.write_png(a.cost_png, heat)
        sums = {f: int(cost[..., i].sum(dtype="u8")) for i, f in enumerate(pkg.hip.COST_FIELDS[:7])}
        print(json.dumps({"cost_frame": a.cost_frame, "cost_field": a.cost_field, "cost_scale": a.cost_scale, "cost_sums": sums,
                          "pixels_over_scale": int(((heat[..., 0] == 255) & (heat[..., 1] == 0)).sum())}))
    if a.aov_png or a.aov_npy:
        aov = tr.render_aov(a.aov_frame)
        if a.aov_npy:
            import numpy as np
            np.save(a.aov_npy, aov)
        if a.aov_png:
            for ch in ("normal", "albedo", "depth", "object"):
                pkg.display.write_png(f"{a.aov_png}_{ch}.png", pkg.display.aov_srgb8(aov, ch))
        hit = aov["hit"] & 3
        print(json.dumps({"aov_frame": a.aov_frame, "pixels": int(aov.size), "miss": int((hit == 0).sum()), "opaque": int((hit == 1).sum()),
                          "glass": int((hit == 2).sum()), "objects_seen": int(len(set(aov["object"][hit != 0].tolist())))}))
    if a.denoise_png:
        n = max(mgr.numAccumulatedFrames - 1, 1)  # frames in the accumulated sum
        fields = {"scale": 1.0 / n}
        if a.denoise_iterations is not None:
            fields["iterations"] = a.denoise_iterations
        if a.denoise_sigma:
            fields["sigmaColour"], fields["sigmaNormal"], fields["sigmaPlane"] = (float(x) for x in a.denoise_sigma.split(","))
        p = api.denoise_params(**fields)
        img = tr.denoise(p, use_accumulated=True, aov_frame=a.aov_frame)
        pkg.display.write_png(a.denoise_png, pkg.display.linear_srgb8(img))
        print(json.dumps({"denoise_png": a.denoise_png, "iterations": p.iterations, "sigma": [p.sigmaColour, p.sigmaNormal, p.sigmaPlane],
                          "demodulate": p.demodulate, "scale": p.scale, "aov_frame": a.aov_frame}))
    if a.vdenoise_png:
        p = api.variance_denoise_params(**({"iterations": a.denoise_iterations} if a.denoise_iterations is not None else {}))
        img = tr.denoise_variance(p, aov_frame=a.aov_frame)
        pkg.display.write_png(a.vdenoise_png, pkg.display.linear_srgb8(img))
        print(json.dumps({"vdenoise_png": a.vdenoise_png, "iterations": p.iterations, "sigma": [p.sigmaLuminance, p.sigmaNormal, p.sigmaPlane],
                          "demodulate": p.demodulate, "unknownVariance": p.unknownVariance, "batches": a.variance_batches, "aov_frame": a.aov_frame}))
    if a.variance_png:
        import numpy as np
        m = tr.read_moments().astype(np.float64)
        nb = m[..., 3]
        known = nb >= 2
        safe = np.where(known, nb, 2.0)
        sd = np.sqrt(np.maximum(m[..., 1] - m[..., 0] * m[..., 0] / safe, 0.0) / (safe * (safe - 1.0)))
        grey = np.clip(sd / a.variance_scale, 0.0, 1.0)
        heat = np.stack([grey, grey, grey], axis=-1)
        heat[sd > a.variance_scale] = (1.0, 0.0, 0.0)
        heat[~known] = (0.0, 0.0, 1.0)
        pkg.display.write_png(a.variance_png, pkg.display.linear_srgb8(heat.astype(np.float32)))
        print(json.dumps({"variance_png": a.variance_png, "batches": a.variance_batches, "scale": a.variance_scale, "median_sd": float(np.median(sd[known])) if known.any() else None,
                          "pixels_over_scale": int((sd > a.variance_scale).sum()), "pixels_unknown": int((~known).sum())}))
    if a.ao_png:
        import numpy as np
        dev = torch.device("cuda:0")
        aov = torch.zeros((h * w, 16), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        tr.render_aov_centre_to_device(aov.data_ptr(), aov.numel() * 4)
        tr.synchronize()
        hit = (aov[:, 7].view(torch.int32) & 3) != 0
        nrm, pos = aov[hit, 1:4], aov[hit, 4:7]
        n = int(hit.sum().item())
        ao = torch.ones(h * w, dtype=torch.float32, device=dev)
        if n:
            extent = float((pos.max(dim=0).values - pos.min(dim=0).values).norm())
            rays = torch.zeros((n, 8), dtype=torch.float32, device=dev)
            rays[:, 0:3] = pos + nrm * (1e-4 * extent)
            rays[:, 3] = a.ao_distance * extent
            occ = torch.zeros(n, dtype=torch.int32, device=dev)
            blocked = torch.zeros(n, dtype=torch.float32, device=dev)
            gen = torch.Generator(device=dev).manual_seed(a.seed)
            for _ in range(a.ao_samples):  # normalize(normal + unit vector): cosine-weighted about the normal
                u = torch.nn.functional.normalize(torch.randn((n, 3), generator=gen, device=dev), dim=-1)
                rays[:, 4:7] = torch.nn.functional.normalize(nrm + 0.999 * u, dim=-1)
                torch.cuda.synchronize()  # torch's stream is not the context's: the rays are complete before the pass reads them
                tr.query_occluded_buffers(rays.data_ptr(), n, occ.data_ptr())
                tr.synchronize()
                blocked += occ.to(torch.float32)
            ao[hit] = 1.0 - blocked / a.ao_samples
        grey = ao.reshape(h, w, 1).expand(h, w, 3).cpu().numpy().astype(np.float32)
        pkg.display.write_png(a.ao_png, pkg.display.linear_srgb8(np.ascontiguousarray(grey)))
        print(json.dumps({"ao_png": a.ao_png, "samples": a.ao_samples, "distance": a.ao_distance, "hit_pixels": n, "rays": n * a.ao_samples,
                          "mean_ao": float(ao[hit].mean().item()) if n else None}))
    if a.panorama_png:
        import math
        import numpy as np
        dev = torch.device("cuda:0")
        n = pano_w * pano_h
        origin = torch.tensor(list(mgr.params().camLocalToWorld)[12:15], dtype=torch.float32, device=dev)  # the camera position
        ys, xs = torch.meshgrid(torch.arange(pano_h, device=dev), torch.arange(pano_w, device=dev), indexing="ij")
        rays = torch.zeros((n, 8), dtype=torch.float32, device=dev)  # RtPathRay: origin, unused, dir, rng
        rays[:, 0:3] = origin
        idx = torch.arange(n, dtype=torch.int64, device=dev)
        state = ((idx + 1) * 747796405 + a.seed * 2891336453) & 0xffffffff  # one generator state per texel; later samples chain the returned one
        rays.view(torch.int32)[:, 7] = torch.where(state >= 1 << 31, state - (1 << 32), state).to(torch.int32)
        out = torch.zeros((n, 4), dtype=torch.float32, device=dev)  # RtRadiance: rgb, rng
        total = torch.zeros((n, 3), dtype=torch.float32, device=dev)
        gen = torch.Generator(device=dev).manual_seed(a.seed)
        for _ in range(a.panorama_samples):
            jit = torch.rand((2, pano_h, pano_w), generator=gen, device=dev)
            lon = ((xs + jit[0]) / pano_w * 2.0 - 1.0) * math.pi  # -pi .. pi, 0 = +z
            lat = (0.5 - (ys + jit[1]) / pano_h) * math.pi        # +pi/2 (up) at the top row
            rays[:, 4] = (torch.cos(lat) * torch.sin(lon)).reshape(n)
            rays[:, 5] = torch.sin(lat).reshape(n)
            rays[:, 6] = (torch.cos(lat) * torch.cos(lon)).reshape(n)
            torch.cuda.synchronize()  # torch's stream is not the context's: the rays are complete before the pass reads them
            tr.radiance_trace_buffers(rays.data_ptr(), n, out.data_ptr())
            tr.synchronize()
            total += out[:, 0:3]
            rays.view(torch.int32)[:, 7] = out.view(torch.int32)[:, 3]  # the next sample goes on where this path's generator stopped
        img = (total / a.panorama_samples).reshape(pano_h, pano_w, 3).flip(0).cpu().numpy().astype(np.float32)  # rows bottom-up, as the frames
        pkg.display.write_png(a.panorama_png, pkg.display.linear_srgb8(np.ascontiguousarray(img)))
        print(json.dumps({"panorama_png": a.panorama_png, "size": [pano_w, pano_h], "samples": a.panorama_samples, "rays": n * a.panorama_samples,
                          "mean_rgb": [float(v) for v in img.reshape(-1, 3).mean(axis=0)]}))
    if a.reproject_png:
        import ctypes as C
        import numpy as np
        hip = C.CDLL("libamdhip64.so")
        d_prev = C.c_void_p()
        if hip.hipMalloc(C.byref(d_prev), C.c_size_t(w * h * 64)) != 0:
            raise RuntimeError("hipMalloc failed")
        if a.reproject_centre:
            tr.render_aov_centre_to_device(d_prev.value, w * h * 64)
        else:
            tr.render_aov_to_device(a.aov_frame, d_prev.value, w * h * 64)
        before = mgr.params()
        t = mgr.camera.transform
        offset = [float(x) for x in a.reproject_move.split(",")]
        mgr.camera.transform = pkg.Transform(tuple(np.array(t.position) + np.array(offset)), t.euler, t.scale)
        mgr.SetShaderParams()
        if a.reproject_centre:
            tr.reproject_accumulated_moving(api.reproject_params(before), d_prev.value, pkg.abi.AOV_CENTRE, None, 0)
        else:
            tr.reproject_accumulated(api.reproject_params(before), d_prev.value, a.aov_frame)
        mgr.RenderFrames(a.reproject_frames)
        img = tr.resolve()
        hip.hipFree(d_prev)
        total = max(mgr.numAccumulatedFrames - 1, 1)
        grey = np.repeat(np.clip(img[..., 3:4] / total, 0, 1) ** 2.2, 3, axis=-1).astype(np.float32)
        pkg.display.write_png(f"{a.reproject_png}_resolved.png", pkg.display.linear_srgb8(img))
        pkg.display.write_png(f"{a.reproject_png}_history.png", pkg.display.linear_srgb8(grey))
        carried = img[..., 3] > a.reproject_frames
        print(json.dumps({"reproject_png": a.reproject_png, "move": offset, "frames_after": a.reproject_frames, "pixels": int(carried.size),
                          "carried": int(carried.sum()), "mean_history": float(img[..., 3].mean())}))


if __name__ == "__main__":
    main()
