"""The calls of include/rt_motion.h on the GPU.  Every comparison of records and images is == on the bit patterns, every pixel, every field
or channel, against the oracle's functions on the NumPy centre rays and against the NumPy restatement of the header's prose
(tests/motion_reference.py).

  A. rt_render_aov_centre*: every field against the oracle on the restated centre rays; no dependence on anything random; agreement with
     rt_render_aov where the jitter is zero; device variant, torch tensor, strip partitions, degenerate images; side effects, errors, watchdog;
  B. rt_reproject_buffers_moving on synthetic views and tables; rt_reproject_accumulated_moving end to end with a model that
     rt_update_models moved, with and without a camera move; the share it carries where the static call carries nothing; errors, watchdog;
  C. it helps: centre records do not lose to jittered ones, and a moving model's history beats a restart."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import motion_reference as mref
import reproject_reference as ref
import aov_support as ga
from gpu_support import DevBuf, assert_same_bits
from reproject_support import NEARBY, move_camera, records_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ---------------------------------------------------------------- A. centre records
CENTRE_CASES = [  # name, scene, W, H, tweaks
    ("config2_flat", (2, {}), 48, 27, {}),
    ("config3_bvh", (3, {}), 37, 23, {}),
    ("config4_dof", (4, {"subdivisions": 3}), 48, 27, {}),
    ("glass_balls", "glass_balls_file", 37, 23, {}),
    ("crowded70_many", "crowded70", 48, 27, {}),
]


@pytest.mark.parametrize("case", CENTRE_CASES, ids=[c[0] for c in CENTRE_CASES])
def test_centre_records_equal_the_oracles_functions_on_the_centre_rays(pkg, api, orc, case):
    name, spec, w, h, tweak = case
    tr, ot = api.create_tracer(0), orc.create_tracer(1)
    try:
        su = ga.Setup(pkg, api, tr, spec, w, h, tweak)
        so = ga.Setup(pkg, orc, ot, spec, w, h, tweak)
        p = su.params(1)
        aov = tr.render_aov_centre()
        assert aov.shape == (h, w) and aov.dtype == pkg.abi.AOV_DTYPE
        origins, dirs = mref.centre_rays(orc, p, w, h)
        want = ga.oracle_records(pkg, orc, ot, so, p, origins, dirs, aov["object"])
        want["triangle"] = aov["triangle"]  # (checked below, as tests/test_gpu_aov.py checks it)
        ga.assert_records_equal(aov, want, name)
        hit = aov["hit"] & 3
        assert np.array_equal(aov["object"] >= 0, hit != 0) and (hit != 0).any()
        dbg = tr.debug_intersect(origins.reshape(-1, 3), dirs.reshape(-1, 3)).reshape(h, w, 10)  # HIP's own intersection of the restated rays
        assert dbg[..., 2].view(np.uint32).tolist() == aov["dst"].view(np.uint32).tolist()
        assert dbg[..., 6:9].view(np.uint32).tolist() == aov["pos"].view(np.uint32).tolist()
        ga.check_triangles(orc, so, aov, origins, dirs)
        if spec == "glass_balls_file":
            assert (hit == 2).any() and (hit == 1).any()
    finally:
        tr.close()
        ot.close()


@pytest.mark.parametrize("w,h", [(1, 9), (9, 1)])
def test_centre_records_of_one_pixel_wide_and_high_images(pkg, api, orc, w, h):
    tr = api.create_tracer(0)
    try:
        su = ga.Setup(pkg, api, tr, (3, {}), w, h)
        aov = tr.render_aov_centre()
        origins, dirs = mref.centre_rays(orc, su.params(1), w, h)
        assert np.isnan(dirs).all() and np.isfinite(origins).all()
        dbg = tr.debug_intersect(origins.reshape(-1, 3), dirs.reshape(-1, 3)).reshape(h, w, 10)
        assert dbg[..., 2].view(np.uint32).tolist() == aov["dst"].view(np.uint32).tolist()
        assert np.array_equal(dbg[..., 0] != 0, (aov["hit"] & 3) != 0)
        assert dbg[..., 3:6].view(np.uint32).tolist() == aov["normal"].view(np.uint32).tolist()
        assert dbg[..., 6:9].view(np.uint32).tolist() == aov["pos"].view(np.uint32).tolist()
    finally:
        tr.close()


def centre_of(pkg, api, spec, w, h, tweak=None, seed=1, frames=0, partition=None):
    tr = api.create_tracer(0)
    try:
        if partition:
            tr.set_partition(*partition)
        su = ga.Setup(pkg, api, tr, spec, w, h, tweak, seed)
        if frames:
            su.mgr.RenderFrames(frames)
        return tr.render_aov_centre(), tr.local_to_global_rows()
    finally:
        tr.close()


@pytest.mark.parametrize("spec", [(3, {}), (2, {})], ids=["bvh", "flat"])
def test_strip_partitions_reassemble_the_centre_records(pkg, api, orc, spec):
    w, h, parts = 37, 52, 3
    full, _ = centre_of(pkg, api, spec, w, h)
    whole, seen = np.zeros_like(full), np.zeros(h, dtype=int)
    for i in range(parts):
        local, rows = centre_of(pkg, api, spec, w, h, partition=(8, i, parts))
        assert local.shape == (len(rows), w)
        whole[rows] = local
        seen[rows] += 1
    assert (seen == 1).all()
    ga.assert_records_equal(whole, full, "8-row strips, 3 parts")
    mt = api.create_multi_tracer([0, 0, 0])
    try:
        ga.Setup(pkg, api, mt, spec, w, h)
        ga.assert_records_equal(mt.render_aov_centre(), full, "MultiTracer.render_aov_centre")
    finally:
        mt.close()


def test_centre_records_depend_on_nothing_random(pkg, api):
    spec, w, h = (4, {"subdivisions": 3}), 64, 36  # the scene with a defocus draw
    base, _ = centre_of(pkg, api, spec, w, h)
    assert ((base["hit"] & 3) != 0).any()
    for kw in (dict(seed=77), dict(frames=5), dict(tweak={"defocusStrength": 0.0}), dict(tweak={"divergeStrength": 0.0}),
               dict(tweak={"defocusStrength": 250.0, "divergeStrength": 9.0}, seed=3, frames=2)):
        other, _ = centre_of(pkg, api, spec, w, h, **kw)
        assert other.tobytes() == base.tobytes(), kw


@pytest.mark.parametrize("spec,frame", [((3, {}), 1), ((2, {}), 7)], ids=["bvh", "flat"])
def test_without_jitter_the_centre_records_are_the_frames_records(pkg, api, orc, spec, frame):
    """defocusStrength = divergeStrength = 0: camera ray 0 of a frame is focusPoint + right * 0 + up * 0 seen from camOrigin + 0.  The
    restated rays decide where that is the centre ray bit for bit (a component -0 of focusPoint becomes +0 by the added zeros); there every
    field of the two records is equal — and that is nearly everywhere."""
    w, h = 48, 27
    tr = api.create_tracer(0)
    try:
        su = ga.Setup(pkg, api, tr, spec, w, h, tweak={"divergeStrength": 0.0, "defocusStrength": 0.0})
        p = su.params(frame)
        oj, dj = ga.camera_rays(orc, p, w, h, frame)
        oc, dc = mref.centre_rays(orc, p, w, h)
        same = (dj.view(np.uint32) == dc.view(np.uint32)).all(axis=-1) & (oj.view(np.uint32) == oc.view(np.uint32)).all(axis=-1)
        print(f"rays bit-equal on {int(same.sum())} of {same.size} pixels")
        assert same.mean() > 0.9
        jit, cen = tr.render_aov(frame), tr.render_aov_centre()
        ga.assert_records_equal(cen[same], jit[same], "centre vs frame records where the rays are the same")
        assert ((cen["hit"] & 3) != 0)[same].any()
    finally:
        tr.close()


def test_centre_device_variant_equals_the_host_variant(pkg, api):
    w, h = 96, 54
    for spec in ((3, {}), (2, {}), "crowded70"):
        tr = api.create_tracer(0)
        d = DevBuf(h * w * 64, fill=0xff)
        try:
            su = ga.Setup(pkg, api, tr, spec, w, h)
            host = tr.render_aov_centre()
            su.mgr.RenderFrames(3)  # frames in flight in front of the pass
            tr.render_aov_centre_to_device(d.ptr, d.nbytes)
            tr.synchronize()
            ga.assert_records_equal(records_of(pkg, d, h, w), host, f"rt_render_aov_centre_to_device vs rt_render_aov_centre ({spec})")
        finally:
            d.free()
            tr.close()


_TORCH_CHILD = r"""
import sys
import numpy as np
import torch
torch.cuda.set_device(0)
root = sys.argv[1]
sys.path.insert(0, root)
import __graft_entry__ as graft
pkg = graft.load_package()
api = pkg.load_library()
w, h = 96, 54
for cfg in (3, 2):
    tr = api.create_tracer(0)
    mgr = pkg.scenes.get(cfg).make_manager(tr, api, w, h)
    mgr.OnEnable(renderSeed=1)
    host = tr.render_aov_centre()
    mgr.RenderFrames(3)
    s = torch.cuda.Stream()
    tr.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        t = torch.full((h, w, 16), 0x7fc00001, dtype=torch.int32, device="cuda:0")
        s.synchronize()
        tr.render_aov_centre_to_device(t.data_ptr(), t.numel() * 4)
        first = t.clone()  # on the caller's stream, behind the pass
    s.synchronize()
    assert first.cpu().numpy().tobytes() == host.tobytes(), "stream order (config %d)" % cfg
    tr.set_stream(None)
    tr.synchronize()
    assert t.cpu().numpy().view(pkg.abi.AOV_DTYPE).reshape(h, w).tobytes() == host.tobytes(), "tensor != host variant (config %d)" % cfg
    tr.close()
print("CENTRE_TORCH_OK")
"""


def test_centre_device_variant_into_a_torch_tensor_on_a_torch_stream(pkg, api):
    p = subprocess.run([sys.executable, "-c", _TORCH_CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "CENTRE_TORCH_OK" in p.stdout, "rc=%d\n%s\n%s" % (p.returncode, p.stdout[-3000:], p.stderr[-3000:])


def test_centre_calls_leave_no_trace(pkg, api):
    w, h = 96, 54
    tr = api.create_tracer(0)
    tr.enable_stats(True)
    t = DevBuf(h * w * 64)
    try:
        su = ga.Setup(pkg, api, tr, (3, {}), w, h, seed=5)
        su.mgr.RenderFrames(17)
        for _ in range(3):
            su.mgr.RenderFrame()  # rt_render_frame may hold these back

        def state():
            c = tr.counters()
            c.pop("gpuMs")
            return tr.frame(), c, tr.read_frame().tobytes(), tr.read_accumulated().tobytes()  # (the reads succeed: the watchdog word is clear)
        s0 = state()
        a = tr.render_aov_centre()
        tr.render_aov_centre_to_device(t.ptr, t.nbytes)
        tr.synchronize()
        assert records_of(pkg, t, h, w).tobytes() == a.tobytes()
        assert state() == s0
        su.mgr.RenderFrames(2)
        assert tr.frame() == s0[0] + 2
    finally:
        tr.close()
        t.free()


def test_centre_errors(pkg, api):
    abi = pkg.abi
    buf = np.zeros((36, 64), dtype=abi.AOV_DTYPE)
    dev = DevBuf(buf.nbytes)
    calls = ((api.render_aov_centre, buf.ctypes.data), (api.render_aov_centre_to_device, dev.ptr))
    tr = api.create_tracer(0)
    try:
        for call, ptr in calls:
            assert call(tr.h, ptr, buf.nbytes) == abi.RT_ERR_STATE  # before rt_resize
        tr.resize(64, 36)
        for call, ptr in calls:
            assert call(tr.h, ptr, buf.nbytes) == abi.RT_ERR_STATE  # before rt_upload_scene
        mgr = ga.scene_of(pkg, (3, {})).make_manager(tr, api, 64, 36)
        mgr.InitTexturesAndBuffers()
        mgr.InitBVH()
        for call, ptr in calls:
            assert call(tr.h, ptr, buf.nbytes) == abi.RT_ERR_STATE  # before rt_set_params
        tr.close()
        tr = api.create_tracer(0)
        ga.Setup(pkg, api, tr, (3, {}), 64, 36)
        for call, ptr in calls:
            assert call(tr.h, ptr, buf.nbytes - 64) == abi.RT_ERR_INVALID_ARG
            assert call(tr.h, ptr, buf.nbytes + 64) == abi.RT_ERR_INVALID_ARG
            assert call(tr.h, None, buf.nbytes) == abi.RT_ERR_INVALID_ARG
        assert api.render_aov_centre_to_device(tr.h, buf.ctypes.data, buf.nbytes) == abi.RT_ERR_INVALID_ARG  # host memory
        assert api.render_aov_centre_to_device(tr.h, dev.ptr + 4, buf.nbytes) == abi.RT_ERR_INVALID_ARG
        assert api.render_aov_centre_to_device(tr.h, dev.ptr + 64, buf.nbytes) == abi.RT_ERR_INVALID_ARG  # runs past the allocation
        for call, ptr in calls:
            assert call(tr.h, ptr, buf.nbytes) == abi.RT_OK
        tr.synchronize()
        assert (buf["hit"] & 3).any()
        ga.assert_records_equal(records_of(pkg, dev, 36, 64), buf, "device vs host")
        # a context that owns part of the image: its rows, like rt_render_aov
        tr.close()
        tr = api.create_tracer(0)
        tr.set_partition(8, 1, 2)
        ga.Setup(pkg, api, tr, (3, {}), 64, 36)
        rows = tr.local_to_global_rows()
        assert 0 < len(rows) < 36 and tr.render_aov_centre().tobytes() == buf[rows].tobytes()
    finally:
        tr.close()
        dev.free()


def test_centre_watchdog_fails_the_pass_not_the_context(pkg, api, monkeypatch):
    """RT_TRAV_LIMIT=4, the hook of tests/test_gpu_aov.py::test_watchdog_fails_the_pass_not_the_context (a software step limit: nothing can
    hang): the host variant says so when it returns, the device variant at the next rt_synchronize, once."""
    tr = api.create_tracer(0)
    t = DevBuf(36 * 64 * 64)
    try:
        monkeypatch.setenv("RT_TRAV_LIMIT", "4")
        ga.Setup(pkg, api, tr, (3, {}), 64, 36)
        monkeypatch.delenv("RT_TRAV_LIMIT")
        with pytest.raises(pkg.abi.RtError) as e:
            tr.render_aov_centre()
        assert e.value.status == pkg.abi.RT_ERR_HIP and "watchdog" in str(e.value) and "rt_render_aov_centre" in str(e.value), str(e.value)
        tr.render_aov_centre_to_device(t.ptr, t.nbytes)  # enqueued: RT_OK
        with pytest.raises(pkg.abi.RtError) as e:
            tr.synchronize()
        assert e.value.status == pkg.abi.RT_ERR_HIP and "watchdog" in str(e.value), str(e.value)
        tr.synchronize()  # reported once
        assert tr.counters()["segments"] == 0 and not tr.read_accumulated().any() and tr.frame() == 1
    finally:
        tr.close()
        t.free()


# ---------------------------------------------------------------- B. the reprojection with a table
def moving_on_device(pkg, tr, rgba, prev, cur, table, p):
    """rt_reproject_buffers_moving on uploaded copies (table: (n, 12) float32 or None); returns the output and the inputs as they are afterwards."""
    h, w = rgba.shape[:2]
    bufs = [DevBuf.of(rgba), DevBuf.of(prev), DevBuf.of(cur), DevBuf(rgba.nbytes, fill=0xff)]
    d_m = DevBuf.of(table) if table is not None and len(table) else None
    try:
        tr.reproject_buffers_moving(w, h, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, d_m.ptr if d_m else None, 0 if d_m is None else len(table), bufs[3].ptr, p)
        tr.synchronize()
        return bufs[3].image(h, w), (bufs[0].image(h, w), records_of(pkg, bufs[1], h, w), records_of(pkg, bufs[2], h, w))
    finally:
        for d in bufs + ([d_m] if d_m else []):
            d.free()


@pytest.mark.parametrize("w,h", [(1, 1), (1, 37), (37, 1), (2, 2), (64, 36), (333, 77)])
def test_reproject_buffers_moving_equals_the_numpy_restatement(pkg, api, orc, w, h):
    """Tables of 1 (objects 1 and 2 lie beyond it), 3 and 200 entries (indexed at 1, 68 and 135) that mix translation, rotation, the
    identity and entries with a NaN or an infinity; no table at all (NULL, 0); every object beyond the table."""
    tr = api.create_tracer(0)  # no scene, no rt_resize
    try:
        for n_case, case in enumerate(sorted(ref.CAMERAS)):
            rgba, prev, cur, cam = ref.synthetic(pkg, w, h, case, seed=w + h)
            far = mref.spread_objects(prev, cur, 67, 1)
            beyond = mref.spread_objects(prev, cur, 1, 3)
            runs = (("3", (prev, cur), mref.table(3)), ("1", (prev, cur), mref.table(1)), ("200", far, mref.table(200)), ("none", (prev, cur), None),
                    ("beyond", beyond, mref.table(3)))
            for n_run, (what, (pv, cu), table) in enumerate(runs):
                fields = dict(maxHistory=16.0) if (n_case + n_run) % 2 else dict(flags=1, maxHistory=1000.0, maxPlaneDistance=0.02, minNormalDot=0.99)
                p = api.reproject_params(prevViewParams=ref.VIEW_PARAMS, prevCamLocalToWorld=cam, **fields)
                got, (rgba2, prev2, cur2) = moving_on_device(pkg, tr, rgba, pv, cu, table, p)
                assert rgba2.tobytes() == rgba.tobytes() and prev2.tobytes() == pv.tobytes() and cur2.tobytes() == cu.tobytes(), "an input was written"
                assert_same_bits(got, mref.reproject_moving_with(orc, rgba, pv, cu, table, p), f"{case} {w} x {h} {fields} table {what}")
                if what in ("none", "beyond"):
                    assert_same_bits(got, ref.reproject_with(orc, rgba, prev, cur, p), f"{case} {w} x {h} table {what}: the static call")
                if w == 1 or h == 1 or case == "behind":
                    assert not got.view(np.uint32).any()
                elif w > 2 and what != "3":
                    assert (got[..., 3] > 0).any()
    finally:
        tr.close()


def moving_end_to_end(pkg, api, w, h, camera=None, bound=False, in_flight=False, after=0, target=None, table_used=True, step=1.0, glass=False):
    """Config 3: 4 frames, the centre records to the device, 3 more frames; the small block most pixels see steps on (rt_update_models),
    the camera moves by `camera` (move_camera's arguments, None: it stays); the table by rt_motion_from_scene from the two model arrays,
    uploaded; rt_reproject_accumulated_moving(RT_AOV_CENTRE).  in_flight: nothing is read back (and so nothing waited for) before the call."""
    tr = api.create_tracer(0)
    n = h * w
    d_prev, d_cur = DevBuf(n * 64, fill=0xff), DevBuf(n * 64, fill=0xff)
    targets = [DevBuf(n * 16), DevBuf(n * 16)] if bound else []
    d_m = None
    try:
        su = ga.Setup(pkg, api, tr, (3, {}), w, h)
        if bound:
            tr.bind_render_targets(targets[0].ptr, targets[1].ptr)
        su.mgr.RenderFrames(4)
        tr.render_aov_centre_to_device(d_prev.ptr, d_prev.nbytes)
        su.mgr.RenderFrames(3)
        p_a = su.mgr.params()
        before = rec_a = None
        if not in_flight:
            before, rec_a = tr.read_accumulated(), tr.render_aov_centre()
            assert records_of(pkg, d_prev, h, w).tobytes() == rec_a.tobytes(), "A's records"
            target = mref.movable_model(su, rec_a, opaque=not glass)
        spheres, models_a = su.scene["spheres"], su.mgr.meshInfo.copy()
        model = su.mgr.models[target - su.n_spheres]
        model.transform = mref.step_model(pkg, model.transform, step)
        su.mgr.UpdateModels()
        table = api.motion_table(spheres, spheres, models_a, su.mgr.meshInfo)
        assert len(table) == su.n_spheres + len(su.mgr.models)
        d_m = DevBuf.of(table)
        if camera is not None:
            move_camera(pkg, su.mgr, **camera)
        p = api.reproject_params(p_a, flags=pkg.abi.REPROJECT_FLAG_GLASS if glass else 0)
        if table_used:
            tr.reproject_accumulated_moving(p, d_prev.ptr, pkg.abi.AOV_CENTRE, d_m.ptr, len(table), d_cur.ptr)
        else:
            tr.reproject_accumulated_moving(p, d_prev.ptr, pkg.abi.AOV_CENTRE, None, 0, d_cur.ptr)
        tr.synchronize()
        got = tr.read_accumulated()
        if bound:
            assert targets[1].image(h, w).tobytes() == got.tobytes(), "the bound AccumulatedRender is the one that was reprojected"
        rec_b = tr.render_aov_centre()
        extra = None
        if after:
            su.mgr.RenderFrames(after)
            extra = tr.read_accumulated()
        return dict(got=got, cur=records_of(pkg, d_cur, h, w), before=before, rec_a=rec_a, rec_b=rec_b, p=p, extra=extra, table=table["m"], target=target)
    finally:
        tr.close()
        for d in [d_prev, d_cur] + targets + ([d_m] if d_m else []):
            d.free()


CAMERA_MOVES = [None, dict(offset=(0.05, 0.02, 0.03), turn=(0.0, 0.4, 0.0))]


@pytest.mark.parametrize("camera", CAMERA_MOVES, ids=["camera_fixed", "camera_moves"])
def test_reproject_accumulated_moving_end_to_end(pkg, api, orc, camera, monkeypatch):
    """The scene of tests/test_gpu_reproject.py::test_a_model_moved_between_the_views_carries_nothing, but not its model: the small model
    most pixels see there is the GLASS block, and a glass first hit carries nothing under the default flags (rule 1), so "more than half
    carried" cannot hold on it.  The block that steps here is the small OPAQUE one (tests/motion_reference.py::movable_model); the glass
    block steps, under flag bit 0, in test_the_glass_block_steps_under_flag_bit_0."""
    w, h = 96, 54
    r = moving_end_to_end(pkg, api, w, h, camera, after=3)
    assert r["cur"].tobytes() == r["rec_b"].tobytes(), "d_cur_aov_out != rt_render_aov_centre after the move"
    assert r["rec_a"].tobytes() != r["rec_b"].tobytes()
    want = mref.reproject_moving_with(orc, r["before"], r["rec_a"], r["rec_b"], r["table"], r["p"])
    assert_same_bits(r["got"], want, "rt_reproject_accumulated_moving")
    # the carried share: a condition on the input (the step was chosen on the CPU: tools/reproject_cpu_check.py --model-step 1), asserted
    # of the restatement's result, which the device equals
    on_model = r["rec_b"]["object"] == r["target"]
    static = ref.reproject_with(orc, r["before"], r["rec_a"], r["rec_b"], r["p"])
    print(f"on the moved model: {int(on_model.sum())} pixels, carried {int((want[..., 3] > 0)[on_model].sum())}, by the static call {int((static[..., 3] > 0)[on_model].sum())}")
    assert on_model.sum() > 20 and (want[..., 3] > 0)[on_model].mean() > 0.5
    assert not static[on_model].view(np.uint32).any()
    others = (r["rec_b"]["object"] >= 0) & ~on_model & ((r["rec_b"]["hit"] & 3) != 2)
    assert (want[..., 3] > 0)[others].mean() > 0.7
    # the static-path call on the device: no table
    s = moving_end_to_end(pkg, api, w, h, camera, table_used=False)
    assert_same_bits(s["got"], static, "no table: the static call")
    assert not s["got"][on_model].view(np.uint32).any()
    # layouts, bound targets, frames in flight
    for layout in ("dense", "pre,arena,cache"):
        monkeypatch.setenv("RT_LAYOUT", layout)
        other = moving_end_to_end(pkg, api, w, h, camera)
        monkeypatch.delenv("RT_LAYOUT")
        assert_same_bits(other["got"], r["got"], f"RT_LAYOUT={layout}")
        assert other["cur"].tobytes() == r["cur"].tobytes()
    for kw in (dict(bound=True), dict(in_flight=True), dict(bound=True, in_flight=True)):
        other = moving_end_to_end(pkg, api, w, h, camera, target=r["target"], **kw)
        assert_same_bits(other["got"], r["got"], f"{kw}")
        assert other["cur"].tobytes() == r["cur"].tobytes()
    # frames rendered afterwards add onto it like the oracle's
    ot = orc.create_tracer(16)
    try:
        so = ga.Setup(pkg, orc, ot, (3, {}), w, h)
        so.mgr.RenderFrames(7)
        model = so.mgr.models[r["target"] - so.n_spheres]
        model.transform = mref.step_model(pkg, model.transform)
        so.mgr.UpdateModels()
        if camera is not None:
            move_camera(pkg, so.mgr, **camera)
        ot.write_accumulated(r["got"])
        so.mgr.RenderFrames(3)
        assert_same_bits(r["extra"], ot.read_accumulated(), "3 frames onto the reprojected sum")
    finally:
        ot.close()
    assert (r["extra"][..., 3] == r["got"][..., 3] + 3).all()


@pytest.mark.parametrize("camera", CAMERA_MOVES, ids=["camera_fixed", "camera_moves"])
def test_the_glass_block_steps_under_flag_bit_0(pkg, api, orc, camera):
    """The model test_a_model_moved_between_the_views_carries_nothing moves — the small model most pixels see, the glass block — with
    RT_REPROJECT_FLAG_GLASS: the accumulator equals the restatement bit for bit, with the table and without it.  How many of its pixels
    carry is printed, not asserted: what is seen through glass moves differently from the glass, which is why the flag is off by default."""
    w, h = 96, 54
    r = moving_end_to_end(pkg, api, w, h, camera, glass=True)
    assert int(r["rec_b"]["hit"][r["rec_b"]["object"] == r["target"]][0]) & 3 == 2, "the stepping model is the glass block"
    assert r["p"].flags == 1 and r["cur"].tobytes() == r["rec_b"].tobytes()
    want = mref.reproject_moving_with(orc, r["before"], r["rec_a"], r["rec_b"], r["table"], r["p"])
    assert_same_bits(r["got"], want, "the glass block, with the table")
    on_model = r["rec_b"]["object"] == r["target"]
    static = ref.reproject_with(orc, r["before"], r["rec_a"], r["rec_b"], r["p"])
    print(f"on the glass block: {int(on_model.sum())} pixels, carried {int((want[..., 3] > 0)[on_model].sum())}, by the static call {int((static[..., 3] > 0)[on_model].sum())}")
    assert on_model.sum() > 20
    s = moving_end_to_end(pkg, api, w, h, camera, glass=True, table_used=False)
    assert_same_bits(s["got"], static, "the glass block, no table: the static call")


def test_a_frame_number_selects_the_pass_of_rt_reproject_accumulated(pkg, api):
    """aov_frame >= 1 with no table is rt_reproject_accumulated, bit for bit, d_cur_aov_out included."""
    w, h = 64, 36
    out = []
    for moving in (False, True):
        tr = api.create_tracer(0)
        d_prev, d_cur = DevBuf(h * w * 64), DevBuf(h * w * 64, fill=0xff)
        try:
            su = ga.Setup(pkg, api, tr, (3, {}), w, h)
            su.mgr.RenderFrames(4)
            tr.render_aov_to_device(2, d_prev.ptr, d_prev.nbytes)
            p = api.reproject_params(su.mgr.params())
            move_camera(pkg, su.mgr)
            if moving:
                tr.reproject_accumulated_moving(p, d_prev.ptr, 3, None, 0, d_cur.ptr)
            else:
                tr.reproject_accumulated(p, d_prev.ptr, 3, d_cur.ptr)
            tr.synchronize()
            out.append((tr.read_accumulated(), records_of(pkg, d_cur, h, w), tr.render_aov(3)))
        finally:
            tr.close()
            d_prev.free()
            d_cur.free()
    assert_same_bits(out[1][0], out[0][0], "aov_frame 3, no table")
    assert out[1][1].tobytes() == out[0][1].tobytes() == out[0][2].tobytes() and (out[0][0][..., 3] > 0).any()


def test_moving_errors(pkg, api):
    abi = pkg.abi
    w, h = 64, 36
    img = np.zeros((h, w, 4), dtype=F)
    n_obj = 5
    d_in, d_out, d_prev, d_cur, d_m = DevBuf(img.nbytes), DevBuf(img.nbytes), DevBuf(h * w * 64), DevBuf(h * w * 64), DevBuf.of(mref.table(n_obj, "identity"))
    ok = api.reproject_params(prevViewParams=ref.VIEW_PARAMS, prevCamLocalToWorld=ref.camera())
    tr = api.create_tracer(0)

    def buffers(p=ok, m=-1, n=n_obj, d=None, hh=h):
        return api.reproject_buffers_moving(tr.h, C.byref(p) if p is not None else None, w, hh, d_in.ptr, d_prev.ptr, d_cur.ptr, d_m.ptr if m == -1 else m, n,
                                            d_out.ptr if d is None else d)

    def accumulated(p=ok, m=-1, n=n_obj, frame=0, prev=None, cur=-1):
        return api.reproject_accumulated_moving(tr.h, C.byref(p) if p is not None else None, d_prev.ptr if prev is None else prev, frame, d_m.ptr if m == -1 else m, n,
                                                d_cur.ptr if cur == -1 else cur)
    try:
        assert accumulated() == abi.RT_ERR_STATE  # before rt_resize
        assert buffers() == abi.RT_OK  # needs no scene and no rt_resize
        ga.Setup(pkg, api, tr, (3, {}), w, h)
        accum_ptr = tr.render_targets()[1]
        for call in (buffers, accumulated):
            assert call(n=-1) == abi.RT_ERR_INVALID_ARG and call(n=(1 << 24) + 1) == abi.RT_ERR_INVALID_ARG
            assert call(m=None) == abi.RT_ERR_INVALID_ARG  # null with n_objects > 0
            assert call(m=d_m.ptr + 4, n=n_obj - 1) == abi.RT_ERR_INVALID_ARG  # misaligned (and inside the allocation: only the alignment decides)
            assert call(m=img.ctypes.data) == abi.RT_ERR_INVALID_ARG  # host memory
            assert call(m=d_m.ptr + 48, n=n_obj) == abi.RT_ERR_INVALID_ARG  # runs past the allocation
            assert call(m=d_m.ptr + 48, n=n_obj - 1) == abi.RT_OK
            assert call(m=None, n=0) == abi.RT_OK and call(n=0) == abi.RT_OK
            assert call(None) == abi.RT_ERR_INVALID_ARG
            assert call(api.reproject_params(struct_size=96)) == abi.RT_ERR_ABI_MISMATCH
            assert call(api.reproject_params(maxHistory=0.0)) == abi.RT_ERR_INVALID_ARG
        assert buffers(m=d_out.ptr, n=4) == abi.RT_ERR_INVALID_ARG  # the table overlaps d_out_rgba
        assert buffers(hh=h // 2, m=d_out.ptr + (h // 2) * w * 16, n=4) == abi.RT_OK  # the other half of that allocation does not
        assert buffers(d=d_in.ptr) == abi.RT_ERR_INVALID_ARG  # (the errors of rt_reproject_buffers)
        assert accumulated(m=accum_ptr, n=4) == abi.RT_ERR_INVALID_ARG  # the table overlaps AccumulatedRender
        assert accumulated(m=d_cur.ptr, n=4) == abi.RT_ERR_INVALID_ARG  # ... d_cur_aov_out
        assert accumulated(m=d_cur.ptr, n=4, cur=None) == abi.RT_OK
        assert accumulated(frame=-1) == abi.RT_ERR_INVALID_ARG and accumulated(frame=-7) == abi.RT_ERR_INVALID_ARG
        assert accumulated(frame=0) == abi.RT_OK and accumulated(frame=1) == abi.RT_OK and accumulated(frame=12) == abi.RT_OK
        for bad in (0, d_prev.ptr + 4, d_prev.ptr + 64, img.ctypes.data, accum_ptr):
            assert accumulated(prev=bad) == abi.RT_ERR_INVALID_ARG
        for bad in (d_cur.ptr + 4, d_cur.ptr + 64, img.ctypes.data, d_prev.ptr, accum_ptr):
            assert accumulated(cur=bad) == abi.RT_ERR_INVALID_ARG
        tr.synchronize()
        tr.close()
        tr = api.create_tracer(0)
        tr.set_partition(8, 0, 2)
        ga.Setup(pkg, api, tr, (3, {}), w, h)
        assert accumulated() == abi.RT_ERR_STATE and buffers() == abi.RT_ERR_STATE
        assert b"part" in api.last_error(tr.h)
        mt = api.create_multi_tracer([0, 0])
        try:
            with pytest.raises(abi.RtError) as e:
                mt.reproject_accumulated_moving()
            assert e.value.status == abi.RT_ERR_STATE
        finally:
            mt.close()
    finally:
        tr.close()
        for d in (d_in, d_out, d_prev, d_cur, d_m):
            d.free()


def test_watchdog_of_the_internal_centre_pass_leaves_the_accumulator_untouched(pkg, api, monkeypatch):
    """As tests/test_gpu_reproject.py's test of rt_reproject_accumulated, with the same hook (RT_TRAV_LIMIT=4, a software step limit)."""
    w, h = 64, 36
    tr = api.create_tracer(0)
    d_prev, d_cur, d_m = DevBuf(h * w * 64), DevBuf(h * w * 64), DevBuf.of(mref.table(16, "identity"))
    try:
        monkeypatch.setenv("RT_TRAV_LIMIT", "4")
        su = ga.Setup(pkg, api, tr, (3, {}), w, h)
        monkeypatch.delenv("RT_TRAV_LIMIT")
        image = ref.sums(w, h, 11)
        tr.write_accumulated(image)
        p = api.reproject_params(su.mgr.params())
        tr.reproject_accumulated_moving(p, d_prev.ptr, pkg.abi.AOV_CENTRE, d_m.ptr, 16, d_cur.ptr)  # enqueued: RT_OK
        with pytest.raises(pkg.abi.RtError) as e:
            tr.synchronize()
        assert e.value.status == pkg.abi.RT_ERR_HIP and "watchdog" in str(e.value), str(e.value)
        tr.synchronize()  # reported once
        assert tr.read_accumulated().tobytes() == image.tobytes()
        assert tr.counters()["segments"] == 0 and tr.frame() == 1
        tr.reproject_accumulated_moving(p, d_prev.ptr, pkg.abi.AOV_CENTRE, d_m.ptr, 16)
        with pytest.raises(pkg.abi.RtError) as e:
            tr.resolve()  # a host read that comes before any rt_synchronize reports it too, once
        assert e.value.status == pkg.abi.RT_ERR_HIP and "watchdog" in str(e.value), str(e.value)
        tr.synchronize()
        assert tr.read_accumulated().tobytes() == image.tobytes()
    finally:
        tr.close()
        for d in (d_prev, d_cur, d_m):
            d.free()


def test_a_set_watchdog_word_stays_as_it_is(pkg, api, monkeypatch):
    w, h = 64, 36
    tr = api.create_tracer(0)
    n = h * w
    d_prev, t, t2, d_m = DevBuf(n * 64), DevBuf(n * 16), DevBuf(n * 16), DevBuf.of(mref.table(16, "identity"))
    try:
        monkeypatch.setenv("RT_TRAV_LIMIT", "4")
        su = ga.Setup(pkg, api, tr, (3, {}), w, h)
        monkeypatch.delenv("RT_TRAV_LIMIT")
        su.mgr.RenderFrames(2)

        def word():
            with pytest.raises(pkg.abi.RtError) as e:
                tr.read_accumulated()
            assert "fired" in str(e.value) and "rt_reset_accumulation" in str(e.value), str(e.value)
            return str(e.value)
        before = word()
        p = api.reproject_params(su.mgr.params())
        with pytest.raises(pkg.abi.RtError):
            tr.render_aov_centre()  # (its own pass is cut short too: its own word, its own report)
        tr.render_aov_centre_to_device(d_prev.ptr, d_prev.nbytes)
        with pytest.raises(pkg.abi.RtError):
            tr.synchronize()
        tr.reproject_accumulated_moving(p, d_prev.ptr, pkg.abi.AOV_CENTRE, d_m.ptr, 16)
        with pytest.raises(pkg.abi.RtError):
            tr.synchronize()
        tr.reproject_buffers_moving(w, h, t.ptr, d_prev.ptr, d_prev.ptr, d_m.ptr, 16, t2.ptr, p)
        tr.synchronize()
        assert word() == before and tr.frame() == 3
    finally:
        tr.close()
        for d in (d_prev, t, t2, d_m):
            d.free()


# ---------------------------------------------------------------- C. it helps
def quality_run(pkg, api, w, h, frames_a, frames_b, mode, camera=None, model_steps=0.0, target=None):
    """mode None: no reprojection (a reset at B, or the truth); "frame1": rt_reproject_accumulated with the records of frame 1 on both
    sides; "centre": rt_reproject_accumulated_moving(RT_AOV_CENTRE) with centre records on both sides — and no table while no model steps,
    so that the records are the only thing that differs from "frame1"; with model_steps, the table of rt_motion_from_scene."""
    tr = api.create_tracer(0)
    d_prev = DevBuf(h * w * 64)
    d_m = None
    try:
        su = ga.Setup(pkg, api, tr, (3, {}), w, h)
        carried = None
        if frames_a:
            su.mgr.RenderFrames(frames_a)
            if mode == "frame1":
                tr.render_aov_to_device(1, d_prev.ptr, d_prev.nbytes)
            else:
                tr.render_aov_centre_to_device(d_prev.ptr, d_prev.nbytes)
        p_a = su.mgr.params()
        spheres, models_a = su.scene["spheres"], su.mgr.meshInfo.copy()
        if target is None:
            target = mref.movable_model(su, tr.render_aov_centre())
        if model_steps:
            model = su.mgr.models[target - su.n_spheres]
            model.transform = mref.step_model(pkg, model.transform, model_steps)
            su.mgr.UpdateModels()
        if camera is not None:
            move_camera(pkg, su.mgr, **camera)
        if mode == "frame1":
            tr.reproject_accumulated(api.reproject_params(p_a), d_prev.ptr, 1)
        elif mode == "centre" and not model_steps:
            tr.reproject_accumulated_moving(api.reproject_params(p_a), d_prev.ptr, pkg.abi.AOV_CENTRE, None, 0)
        elif mode == "centre":
            table = api.motion_table(spheres, spheres, models_a, su.mgr.meshInfo)
            d_m = DevBuf.of(table)
            tr.reproject_accumulated_moving(api.reproject_params(p_a), d_prev.ptr, pkg.abi.AOV_CENTRE, d_m.ptr, len(table))
        if mode:
            carried = tr.read_accumulated()[..., 3] > 0
        su.mgr.RenderFrames(frames_b)
        return tr.resolve()[..., :3].astype(np.float64), carried, tr.render_aov_centre(), target
    finally:
        tr.close()
        d_prev.free()
        if d_m:
            d_m.free()


@pytest.mark.parametrize("move", ["nearby", "default"])
def test_centre_records_do_not_lose_to_jittered_ones(pkg, api, move):
    """Config 3 at 320 x 180, the protocol of tests/test_gpu_reproject.py::test_it_reprojects: 32 frames at A, the move, the reprojection, 4
    frames, rt_resolve, against 1,024 frames at B; once with the records of frame 1 on both sides (the yardstick) and once with centre
    records on both sides.  Over the pixels carried in both runs mse_centre <= mse_jittered, for the NEARBY move (0.06 units, 0.4 degrees)
    and for move_camera's default (0.3 units, 2 degrees).  Both ratios to a reset are printed; whether the 2 degree ratio drops below 1 is
    asserted with the room the measurement left.  Measured on an MI355X (profiles/r09_motion.txt): nearby, jittered 0.3307 and centre
    0.1105 of a reset's mse; default, jittered 0.4187 and centre 0.1372 — so the 2 degree ratio is below 1 with either kind of record at this
    size, and the bound asserted for it is halfway between 0.1372 and 1."""
    w, h = 320, 180
    camera = NEARBY if move == "nearby" else {}
    truth, _, _, _ = quality_run(pkg, api, w, h, 0, 1024, None, camera)
    reset, _, _, _ = quality_run(pkg, api, w, h, 0, 4, None, camera)
    jit, carried_j, _, _ = quality_run(pkg, api, w, h, 32, 4, "frame1", camera)
    cen, carried_c, _, _ = quality_run(pkg, api, w, h, 32, 4, "centre", camera)
    both = carried_j & carried_c
    mse = lambda img: float(((img - truth)[both] ** 2).mean())
    mse_j, mse_c, mse_r = mse(jit), mse(cen), mse(reset)
    print(f"{move}: carried jittered {int(carried_j.sum())}, centre {int(carried_c.sum())}, both {int(both.sum())}; mse jittered {mse_j:.6g}, centre {mse_c:.6g}, "
          f"reset {mse_r:.6g}; ratio to a reset: jittered {mse_j / mse_r:.4f}, centre {mse_c / mse_r:.4f}")
    assert both.sum() > 0.5 * both.size * 0.5 and np.isfinite(mse_c)
    assert mse_c <= mse_j
    if move == "default":  # measured 0.1372 (profiles/r09_motion.txt): the bound is halfway between that and 1
        assert mse_c < 0.5686 * mse_r


def test_it_carries_a_moving_model(pkg, api):
    """The same protocol with the camera fixed and the small block most pixels see stepping (tests/motion_reference.py::step_model): over
    the carried pixels on that block, mse(32 carried + 4) < mse(reset + 4) against 1,024 frames of the moved scene — carrying must not be
    worse than restarting.  Measured on an MI355X (profiles/r09_motion.txt): carried 1,162 of the 1,182 pixels on the block, mse 0.01165
    against 0.1061, ratio 0.1098; the bound asserted is halfway between that and 1."""
    w, h = 320, 180
    truth, _, aov, target = quality_run(pkg, api, w, h, 0, 1024, None, model_steps=1.0)
    reset, _, _, _ = quality_run(pkg, api, w, h, 0, 4, None, model_steps=1.0, target=target)
    moved, carried, _, _ = quality_run(pkg, api, w, h, 32, 4, "centre", model_steps=1.0, target=target)
    on = (aov["object"] == target) & carried
    total = int((aov["object"] == target).sum())
    mse_c = float(((moved - truth)[on] ** 2).mean())
    mse_r = float(((reset - truth)[on] ** 2).mean())
    print(f"moving model: carried {int(on.sum())} of {total} pixels on it; mse(32 carried + 4) = {mse_c:.6g}, mse(reset + 4) = {mse_r:.6g}, ratio = {mse_c / mse_r:.4f}")
    assert on.sum() > 0.5 * total
    assert np.isfinite(mse_c) and mse_c < 0.555 * mse_r
