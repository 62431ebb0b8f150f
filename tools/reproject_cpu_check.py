#!/usr/bin/env python3
"""The measurement of tests/test_gpu_reproject.py::test_it_reprojects without a GPU, at a reduced size: the oracle's images through the
NumPy restatement of include/rt_reproject.h (tests/reproject_reference.py).  This is how section 1 of profiles/r08_reproject.txt was made.

Config 3: 32 frames at view A; the records of A; the camera moved by --move times (0.25, 0.1, 0.15) and (0, 2, 0) degrees; the records of
B; the restatement with the library's default parameters; rt_write_accumulated; 4 more frames; the per-pixel divide.  Against the mean of
--truth frames at B, over the pixels with carried history: the mse of that image, of "reset at B + 4 frames", their ratio, the same for
the median and for the mean without the worst 1 % of the pixels.

The oracle has no AOV pass.  The records are made as tests/test_gpu_aov.py makes its expectation: camera ray 0 of frame 1 restated
(camera_rays), oracle_ray_collision per ray.  That call does not name the object it hit; the object is named here by geometry — the sphere
whose surface holds the hit point, else the model with the smallest world box around it — which is good enough to tell the walls, the
light panel and the two blocks of config 3 apart.

--records centre makes both views' records from the unjittered pixel centre (rt_render_aov_centre of include/rt_motion.h, restated in
tests/motion_reference.py) instead of camera ray 0 of frame 1.  --model-step S also moves the small block most pixels see by S steps of
tests/motion_reference.py::step_model between the views, builds the table with rt_motion_from_scene (host code) and carries the image
through the restatement of rt_reproject_buffers_moving; the output then also has the share of the pixels on that block that carry
history, with the table and without it (the static call), and the two mse over the carried pixels on the block.  This is how section 1 of
profiles/r09_motion.txt was made and how the step of tests/test_gpu_motion.py was chosen.

    python tools/reproject_cpu_check.py --size 96x54 --truth 256 --move 0.2
    python tools/reproject_cpu_check.py --size 96x54 --truth 256 --move 0 --records centre --model-step 1
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
import motion_reference as mref  # noqa: E402
import reproject_reference as ref  # noqa: E402
import aov_support as ga  # noqa: E402

SPEC = (3, {})
OFFSET, TURN = np.array([0.25, 0.1, 0.15]), np.array([0.0, 2.0, 0.0])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", default="96x54")
    ap.add_argument("--truth", type=int, default=256, help="frames of the reference image at B")
    ap.add_argument("--move", type=float, default=0.2, help="multiple of the offset (0.25, 0.1, 0.15) and the turn (0, 2, 0) degrees")
    ap.add_argument("--frames-a", type=int, default=32)
    ap.add_argument("--frames-b", type=int, default=4)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--records", choices=("frame1", "centre"), default="frame1", help="the ray both views' records are made from")
    ap.add_argument("--model-step", type=float, default=0.0, help="steps (tests/motion_reference.py::step_model) the most visible small block moves between the views")
    a = ap.parse_args()
    w, h = (int(x) for x in a.size.split("x"))
    pkg, orc = graft.load_package(), graft.load_oracle()
    api = pkg.load_library()  # for rt_reproject_default_params alone: no device is opened

    def move(mgr):
        t = mgr.camera.transform
        mgr.camera.transform = pkg.Transform(tuple(np.array(t.position) + OFFSET * a.move), tuple(np.array(t.euler) + TURN * a.move))
        mgr.SetShaderParams()
        if a.model_step:
            model = mgr.models[target[0] - len(mgr.spheres)]
            model.transform = mref.step_model(pkg, model.transform, a.model_step)
            mgr.UpdateModels()
    target = [None]  # the object that moves (--model-step): named once view A's records exist

    def name_objects(su):
        spheres = [(np.array(s.centre, dtype=np.float64), float(s.radius)) for s in su.mgr.spheres]
        boxes = []
        for m in su.mgr.models:
            v = np.asarray(m.Mesh.vertices, dtype=np.float64).reshape(-1, 3)
            mat = m.transform.localToWorldMatrix
            wv = v @ mat[:3, :3].T + mat[:3, 3]
            boxes.append((wv.min(0) - 2e-3, wv.max(0) + 2e-3))

        def name(pos):
            pos = pos.astype(np.float64)
            for i, (c, r) in enumerate(spheres):
                if abs(np.linalg.norm(pos - c) - r) < 2e-3 * max(r, 1):
                    return i
            best, volume = len(spheres) + len(boxes), np.inf
            for i, (lo, hi) in enumerate(boxes):
                if (pos >= lo).all() and (pos <= hi).all() and np.prod(hi - lo) < volume:
                    best, volume = len(spheres) + i, np.prod(hi - lo)
            return best
        return name

    def records(su, ot):
        name = name_objects(su)
        p = su.params(1)
        origins, dirs = mref.centre_rays(orc, p, w, h) if a.records == "centre" else ga.camera_rays(orc, p, w, h, 1)
        rec = np.zeros((h, w), dtype=pkg.abi.AOV_DTYPE)
        out10 = (C.c_float * 10)()
        for idx in np.ndindex(rec.shape):
            orc.ray_collision(ot.h, ga.F3(*origins[idx]), ga.F3(*dirs[idx]), out10)
            r = np.array(out10[:], dtype=np.float32)
            if r[0] != 0:
                rec[idx]["normal"], rec[idx]["pos"], rec[idx]["object"] = r[3:6], r[6:9], name(r[6:9])
                rec[idx]["hit"] = 2 if int(r[9]) == pkg.abi.MATERIAL_GLASS else 1
            else:
                rec[idx]["object"] = -1
        return rec, p

    def at_b(frames):
        ot = orc.create_tracer(a.threads)
        try:
            su = ga.Setup(pkg, orc, ot, SPEC, w, h)
            move(su.mgr)
            su.mgr.RenderFrames(frames)
            return ot.read_accumulated()[..., :3].astype(np.float64) / frames
        finally:
            ot.close()
    t0 = time.time()
    ot = orc.create_tracer(a.threads)
    try:
        su = ga.Setup(pkg, orc, ot, SPEC, w, h)
        su.mgr.RenderFrames(a.frames_a)
        acc_a = ot.read_accumulated().copy()
        rec_a, p_a = records(su, ot)
        table = static = None
        if a.model_step:
            target[0] = mref.movable_model(su, rec_a)
            spheres, models_a = su.scene["spheres"], su.mgr.meshInfo.copy()
        move(su.mgr)
        rec_b, _ = records(su, ot)
        if a.model_step:
            table = api.motion_table(spheres, spheres, models_a, su.mgr.meshInfo)["m"]
            static = ref.reproject_with(orc, acc_a, rec_a, rec_b, api.reproject_params(p_a))
        carried = mref.reproject_moving_with(orc, acc_a, rec_a, rec_b, table, api.reproject_params(p_a))
        ot.write_accumulated(carried)
        su.mgr.RenderFrames(a.frames_b)
        got = ref.resolve(orc, ot.read_accumulated())[..., :3].astype(np.float64)
    finally:
        ot.close()
    reset, truth = at_b(a.frames_b), at_b(a.truth)
    has, hit = carried[..., 3] > 0, rec_b["object"] >= 0
    e_c, e_r = ((got - truth) ** 2).mean(axis=-1)[has], ((reset - truth) ** 2).mean(axis=-1)[has]
    drop = max(len(e_c) // 100, 1)
    out = {"tool": "reproject_cpu_check", "records": a.records, "size": [w, h], "truth_frames": a.truth, "move": a.move, "offset": (OFFSET * a.move).tolist(), "turn_deg": (TURN * a.move).tolist(),
           "carried": int(has.sum()), "hit": int(hit.sum()), "mse_carried": float(e_c.mean()), "mse_reset": float(e_r.mean()), "ratio": float(e_c.mean() / e_r.mean()),
           "median_carried": float(np.median(e_c)), "median_reset": float(np.median(e_r)),
           "trimmed_carried": float(np.sort(e_c)[:-drop].mean()), "trimmed_reset": float(np.sort(e_r)[:-drop].mean()), "seconds": time.time() - t0}
    if a.model_step:
        on = rec_b["object"] == target[0]
        both = on & has
        e2_c, e2_r = ((got - truth) ** 2).mean(axis=-1)[both], ((reset - truth) ** 2).mean(axis=-1)[both]
        out.update({"model_step": a.model_step, "moved_object": target[0], "on_model": int(on.sum()), "on_model_carried": int(both.sum()),
                    "on_model_carried_by_the_static_call": int((on & (static[..., 3] > 0)).sum()),
                    "on_model_mse_carried": float(e2_c.mean()), "on_model_mse_reset": float(e2_r.mean()), "on_model_ratio": float(e2_c.mean() / e2_r.mean())})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
