"""rt_radiance_trace / rt_radiance_trace_buffers (include/rt_radiance.h) on the GPU: Trace for caller-made rays.  Every oracle comparison
is == on the bit patterns (uint32 views: NaN and -0 count), every ray.

  1. camera equivalence: numRaysPerPixel = 1; rgb of (camera ray, generator state after its two circle draws — restated in
     tests/radiance_reference.py) == oracle_trace_pixel(x, y, F) for every pixel, at 24 x 16 (six blocks) and 9 x 7 (one partial
     block), on config 2 (FLAT), config 3 (BVH), glass_balls and the 70-model scene of tests/test_gpu_query.py (MANY), with defocus and
     diverge both zero and both non-zero, maxBounceCount at the scene's default and at 1; the oracle's values are asserted finite first;
  2. the returned state: numRaysPerPixel = 2; ray 1 made from ray 0's returned rng; ((0 + L0) + L1) / 2 == oracle_trace_pixel;
  3. arbitrary rays (the mix of tests/query_support.py's make_rays), maxBounceCount = 0: a miss gives oracle_environment_light(dir)
     with useSky and 0 without, an opaque hit its emission, a glass hit 0; hit or miss from oracle_ray_collision;
  4. independence: 333 rays in order, reversed and as prefixes n = 1, 63, 64, 65, 130, with a sentinel behind the last record;
  5. RT_GRID=2: the blocks come from the counter, the bits are the same;
  6. the buffer form: torch tensors on a torch stream (a child process), updates made before the call, held-back frames;
  7. no visible state change;  8. every row of the header's error list and both state errors;  9. the pass's own watchdog word."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import query_support as tq  # noqa: E402  (scenes, the ray mix and the cached oracle records: shared, never written)
import radiance_reference as rr  # noqa: E402
from flush_table import held_at  # noqa: E402
from gpu_support import DevBuf  # noqa: E402
from radiance_reference import FRAME, NO_DOF, assert_rgb, params_of  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
F3 = C.c_float * 3
DOF = dict(defocusStrength=40.0, divergeStrength=1.5, focusDistance=4.0)

_SCENES = {}
_CASES = {}


def scene(pkg, api, name):
    """tests/query_support.py's Scene (description and the arrays rt_upload_scene takes), built once per name."""
    if name not in _SCENES:
        _SCENES[name] = tq.Scene(pkg, api, name)
    return _SCENES[name]


def hip_tracer(api, sc, p):
    """Scene and parameters, nothing else: never resized."""
    tr = sc.upload(api.create_tracer(0))
    tr.set_params(p)
    return tr


def camera_case(pkg, api, orc, name, w, h, dof, bounce, spp=1, sky=None):
    """Parameters, the restated camera rays of frame FRAME with their states, and the oracle's pixels: computed once, never written.
    sky: None = the scene's own setting."""
    key = (name, w, h, dof, bounce, spp, sky)
    if key not in _CASES:
        sc = scene(pkg, api, name)
        tweak = dict(DOF if dof else NO_DOF, numRaysPerPixel=spp)
        if bounce is not None:
            tweak["maxBounceCount"] = bounce
        if sky is not None:
            tweak["useSky"] = sky
        p = params_of(sc, api, w, h, tweak)
        ot = orc.create_tracer(1)
        try:
            ot.resize(w, h)
            sc.upload(ot)
            ot.set_params(p)
            want = rr.oracle_pixels(orc, ot, w, h, FRAME)
        finally:
            ot.close()
        origins, dirs, states = rr.camera_rays(orc, p, w, h, FRAME)
        for a in (want, origins, dirs, states):
            a.setflags(write=False)
        _CASES[key] = (sc, p, origins, dirs, states, want)
    return _CASES[key]


# ---------------------------------------------------------------- 1. camera equivalence
@pytest.mark.parametrize("bounce", [None, 1], ids=["bounce_default", "bounce_1"])
@pytest.mark.parametrize("dof", [False, True], ids=["pinhole", "dof"])
@pytest.mark.parametrize("size", [(24, 16), (9, 7)], ids=["24x16", "9x7"])
@pytest.mark.parametrize("name", tq.SCENES)
def test_camera_rays_give_the_oracles_pixels(pkg, api, orc, name, size, dof, bounce):
    w, h = size
    # the scene as it is; and, where it has no sky (few pixels of a small image see an emitter then), once more under the sky
    for sky in (None, True):
        sc, p, origins, dirs, states, want = camera_case(pkg, api, orc, name, w, h, dof, bounce, sky=sky)
        assert np.isfinite(want).all(), "the oracle's pixels of this case are not all finite"
        assert p.numRaysPerPixel == 1 and (p.defocusStrength != 0) == dof and (p.divergeStrength != 0) == dof
        tr = hip_tracer(api, sc, p)
        try:
            rays = pkg.abi.make_path_rays(origins.reshape(-1, 3), dirs.reshape(-1, 3), states.reshape(-1))
            got = tr.radiance_trace(rays)
        finally:
            tr.close()
        assert got.dtype == pkg.abi.RADIANCE_DTYPE and got.shape == (w * h,)
        lit = int((want.reshape(-1, 3) != 0).any(axis=1).sum())
        print(f"{name} {w}x{h} dof={dof} bounce={p.maxBounceCount} sky={p.useSky}: {lit} lit pixels of {w * h}")
        assert_rgb(got["rgb"], want, f"{name} {w}x{h} sky={p.useSky}")
        assert (got["rng"] != states.reshape(-1)).any(), "no path drew a number"
        if p.useSky:
            break


# ---------------------------------------------------------------- 2. the returned state
@pytest.mark.parametrize("name", ["config2_flat", "config3_bvh"])
def test_the_returned_state_chains_the_next_sample(pkg, api, orc, name):
    w, h = 16, 8
    sc, p, origins, dirs, states, want = camera_case(pkg, api, orc, name, w, h, True, None, spp=2)
    assert p.numRaysPerPixel == 2 and np.isfinite(want).all()
    abi = pkg.abi
    tr = hip_tracer(api, sc, p)
    try:
        first = tr.radiance_trace(abi.make_path_rays(origins.reshape(-1, 3), dirs.reshape(-1, 3), states.reshape(-1)))
        o1, d1, s1 = rr.camera_rays(orc, p, w, h, start=first["rng"].reshape(h, w))  # RC:565-576 of sample 1: two more circle draws
        second = tr.radiance_trace(abi.make_path_rays(o1.reshape(-1, 3), d1.reshape(-1, 3), s1.reshape(-1)))
    finally:
        tr.close()
    total = (np.zeros_like(first["rgb"]) + first["rgb"]) + second["rgb"]  # RC:578, fp32, in sample order
    assert_rgb(rr.divide(orc, total, F(2)), want, name)  # RC:581
    assert (first["rgb"] != second["rgb"]).any()


# ---------------------------------------------------------------- 3. arbitrary rays, first segment
@pytest.mark.parametrize("sky", [True, False], ids=["sky", "no_sky"])
@pytest.mark.parametrize("name", tq.SCENES)
def test_first_segment_of_arbitrary_rays(pkg, api, orc, name, sky):
    sc, origins, dirs, want10 = tq.case(pkg, api, orc, name)
    abi = pkg.abi
    p = params_of(sc, api, 64, 36, dict(maxBounceCount=0, useSky=sky))
    n = len(origins)
    hit = want10[:, 0] != 0
    tr = hip_tracer(api, sc, p)
    try:
        seeds = (np.arange(n, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32)
        got = tr.radiance_trace(abi.make_path_rays(origins, dirs, seeds))
        objects = tr.query_closest(abi.make_rays(origins, dirs))["object"]
    finally:
        tr.close()
    assert np.array_equal(objects >= 0, hit)
    want = np.zeros((n, 3), dtype=F)
    out3 = F3()
    with np.errstate(all="ignore"):
        for i in range(n):
            if not hit[i]:
                if sky:
                    orc.environment_light(C.byref(p), F3(*dirs[i]), out3)
                    want[i] = F(0) + F(1) * np.array(out3[:], dtype=F)  # RC:490: incomingLight += GetEnvironmentLight * rayColour
            elif want10[i, 9] != abi.MATERIAL_GLASS:
                m = sc.materials[int(objects[i])]
                assert int(m["flag"]) == int(want10[i, 9])
                want[i] = F(0) + (m["emissionCol"][:3] * m["emissionStrength"]) * F(1)  # RC:530-531
    assert_rgb(got["rgb"], want, f"{name} sky={sky}")
    glass = hit & (want10[:, 9] == abi.MATERIAL_GLASS)
    assert not got["rgb"][glass].any()
    if sky:
        assert got["rgb"][~hit].any()
    else:
        assert not got["rgb"][~hit].any()
    if name in ("crowded70_many", "glass_balls"):
        assert glass.any()
    # a miss draws nothing; a hit draws
    assert np.array_equal(got["rng"][~hit], seeds[~hit]) and (got["rng"][hit] != seeds[hit]).all()


# ---------------------------------------------------------------- 4. independence
@pytest.mark.parametrize("name", ["config2_flat", "config3_bvh", "crowded70_many"])
def test_a_record_depends_on_its_own_ray_only(pkg, api, orc, name):
    w, h = 24, 16
    sc, p, origins, dirs, states, want = camera_case(pkg, api, orc, name, w, h, True, None)
    abi = pkg.abi
    n = 333
    rays = abi.make_path_rays(origins.reshape(-1, 3), dirs.reshape(-1, 3), states.reshape(-1))[:n]
    tr = hip_tracer(api, sc, p)
    try:
        full = tr.radiance_trace(rays)
        assert_rgb(full["rgb"], want.reshape(-1, 3)[:n], name)
        assert tr.radiance_trace(rays[::-1])[::-1].tobytes() == full.tobytes(), "reversed"
        d_rays = DevBuf(n * 32).upload(rays)
        for k in (1, 63, 64, 65, 130):
            assert tr.radiance_trace(rays[:k]).tobytes() == full[:k].tobytes(), k
            d_out = DevBuf(k * 16 + 16, fill=0xa5)
            tr.radiance_trace_buffers(d_rays.ptr, k, d_out.ptr)
            tr.synchronize()
            raw = d_out.download(np.uint8)
            assert raw[:k * 16].tobytes() == full[:k].tobytes() and (raw[k * 16:] == 0xa5).all(), k
            d_out.free()
        d_rays.free()
    finally:
        tr.close()


# ---------------------------------------------------------------- 5. waves go round
def test_a_grid_of_two_waves_draws_its_blocks_from_the_counter(pkg, api, orc, monkeypatch):
    w, h = 24, 16
    sc, p, origins, dirs, states, want = camera_case(pkg, api, orc, "config3_bvh", w, h, False, None)
    rays = pkg.abi.make_path_rays(origins.reshape(-1, 3), dirs.reshape(-1, 3), states.reshape(-1))
    monkeypatch.setenv("RT_GRID", "2")  # read at rt_create: six blocks, two waves
    tr = api.create_tracer(0)
    monkeypatch.delenv("RT_GRID")
    try:
        sc.upload(tr)
        tr.set_params(p)
        got = tr.radiance_trace(rays)
    finally:
        tr.close()
    assert_rgb(got["rgb"], want, "RT_GRID=2")


# ---------------------------------------------------------------- 6. the buffer form
def test_buffer_form_sees_updates_and_runs_behind_held_back_frames(pkg, api, orc, forced=False):
    """A pass enqueued right behind rt_update_spheres and rt_set_params sees both; passes between rt_render_frame calls that are held
    back leave the image what the same frames give without any pass."""
    abi = pkg.abi
    w, h = 64, 36
    images = []
    for with_passes in (True, False):
        tr = api.create_tracer(0)
        try:
            mgr = pkg.scenes.get(2).make_manager(tr, api, w, h)
            mgr.OnEnable(renderSeed=3)
            spheres = mgr._pack_spheres()
            c, r = spheres["centre"][0].astype(np.float64), float(spheres["radius"][0])
            moved = c + [3 * r, 0, 0]
            # rays that graze past sphere 0 where it stands and meet it head on once it has moved
            rays = np.repeat(abi.make_path_rays([moved + [0, 0, -50 * r]], [[0, 0, 1]], 9), 70)
            rays["rng"] = np.arange(70) + 100
            d_rays, d_out = DevBuf(rays.nbytes).upload(rays), DevBuf(70 * 16)
            if with_passes:
                before = tr.radiance_trace(rays)
            mgr.RenderFrames(5)
            for _ in range(3):  # rt_render_frame may hold these back
                mgr.RenderFrame()
                if with_passes:
                    held_at(tr, "test_gpu_radiance: rt_radiance_trace_buffers behind rt_render_frame", forced)
                    tr.radiance_trace_buffers(d_rays.ptr, 70, d_out.ptr)
            if with_passes:
                tr.synchronize()
                assert d_out.download(abi.RADIANCE_DTYPE).tobytes() == before.tobytes()
                spheres["centre"][0] = moved
                spheres["material"]["emissionCol"][0] = (0.5, 0.25, 0.125, 1)
                spheres["material"]["emissionStrength"][0] = 2.0
                spheres["material"]["flag"][0] = 0
                tr.update_spheres(spheres)
                p = mgr.params()
                p.maxBounceCount = 0
                tr.set_params(p)
                tr.radiance_trace_buffers(d_rays.ptr, 70, d_out.ptr)  # no synchronise in between
                tr.synchronize()
                seen = d_out.download(abi.RADIANCE_DTYPE)
                assert (seen["rgb"] == np.array([1.0, 0.5, 0.25], dtype=F)).all(), seen["rgb"][0]  # the moved sphere's emission, one segment
                assert seen.tobytes() == tr.radiance_trace(rays).tobytes(), "buffer form vs host form"
                spheres = mgr._pack_spheres()
                tr.update_spheres(spheres)  # back, for the frames that follow
                mgr.SetShaderParams()
            mgr.RenderFrames(4)
            images.append((tr.read_accumulated().tobytes(), tr.read_frame().tobytes(), tr.frame()))
            d_rays.free(), d_out.free()
        finally:
            tr.close()
    assert images[0] == images[1]


def test_buffer_form_runs_behind_frames_that_are_held_back_for_certain(pkg, api, orc, monkeypatch):
    """The same with RT_HOLD_BACK=1: every rt_render_frame of the burst IS held back (asserted right before each pass)."""
    monkeypatch.setenv("RT_HOLD_BACK", "1")
    test_buffer_form_sees_updates_and_runs_behind_held_back_frames(pkg, api, orc, forced=True)


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
abi = pkg.abi
rng = np.random.default_rng(5)
for cfg in (3, 2):
    tr = api.create_tracer(0)
    mgr = pkg.scenes.get(cfg).make_manager(tr, api, 64, 36)
    mgr.InitBVH()  # the scene ...
    mgr.SetShaderParams()  # ... and the parameters, no image
    n = 1000
    o = rng.normal(size=(n, 3)); o = 12 * o / np.linalg.norm(o, axis=1, keepdims=True) + [0, 1, 0]
    d = rng.uniform(-2, 2, (n, 3)) + [0, 1, 0] - o
    rays = abi.make_path_rays(o, d, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))
    host = tr.radiance_trace(rays)
    assert host["rgb"].any() and (host["rng"] != rays["rng"]).any()
    t_rays = torch.from_numpy(rays.view(np.uint32).reshape(n, 8).copy().view(np.int32)).to("cuda:0")
    t_out = torch.full((n, 4), 0x7fc00001, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    tr.radiance_trace_buffers(t_rays.data_ptr(), n, t_out.data_ptr())
    tr.synchronize()
    assert t_out.cpu().numpy().tobytes() == host.tobytes(), "tensor != host form (config %d)" % cfg
    # on the caller's stream (rt_set_stream): work enqueued on that stream behind the pass sees its records
    s = torch.cuda.Stream()
    tr.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        t2 = torch.zeros((n, 4), dtype=torch.int32, device="cuda:0")
        s.synchronize()
        tr.radiance_trace_buffers(t_rays.data_ptr(), n, t2.data_ptr())
        copy = t2.clone()
    s.synchronize()
    assert copy.cpu().numpy().tobytes() == host.tobytes(), "stream order (config %d)" % cfg
    tr.set_stream(None)
    tr.synchronize()
    tr.close()
print("RADIANCE_TORCH_OK")
"""


def test_buffer_form_into_torch_tensors(pkg, api):
    """rt_radiance_trace_buffers on torch tensors' data_ptr()s == the host form, and in the order of a torch stream given to
    rt_set_stream.  In a child process that imports torch first, so that the library shares torch's HIP runtime."""
    p = subprocess.run([sys.executable, "-c", _TORCH_CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "RADIANCE_TORCH_OK" in p.stdout, "rc=%d\n%s\n%s" % (p.returncode, p.stdout[-3000:], p.stderr[-3000:])


# ---------------------------------------------------------------- 7. no visible state change
def mixed_calls(tr, rays, bufs):
    d_rays, d_out = bufs
    n = len(rays)
    out = tr.radiance_trace(rays)
    tr.radiance_trace_buffers(d_rays.ptr, n, d_out.ptr)
    tr.synchronize()
    assert d_out.download(np.uint8).tobytes() == out.tobytes()
    assert tr.radiance_trace(rays[:0]).shape == (0,)
    return out


def test_radiance_calls_leave_no_trace(pkg, api, orc):
    w, h = 24, 16
    sc, p, origins, dirs, states, want = camera_case(pkg, api, orc, "config3_bvh", w, h, True, None)
    rays = pkg.abi.make_path_rays(origins.reshape(-1, 3), dirs.reshape(-1, 3), states.reshape(-1))
    n = len(rays)
    bufs = (DevBuf(n * 32).upload(rays), DevBuf(n * 16))
    try:
        # a rendering context, whole and as part 1 of 2 of a strip partition: everything a caller can read is the same before and after
        for part in (None, 1):
            tr = api.create_tracer(0)
            tr.enable_stats(True)
            if part is not None:
                tr.set_partition(8, part, 2)
            mgr = pkg.scenes.get(3).make_manager(tr, api, 64, 40)
            mgr.OnEnable(renderSeed=5)
            mgr.RenderFrames(4)
            tr.variance_update()
            mgr.RenderFrames(4)
            tr.variance_update()
            tr.adaptive_select(tr.adaptive_params(threshold=0.01, minFrames=0))
            mgr.RenderFrame()
            before = tq.snapshot(tr)
            assert before["counters"]["segments"] > 0
            got = mixed_calls(tr, rays, bufs)
            after = tq.snapshot(tr)
            assert before == after, [k for k in before if before[k] != after[k]]
            assert got["rgb"].any()
            tr.close()
    finally:
        for b in bufs:
            b.free()


# ---------------------------------------------------------------- 8. errors and state
def test_errors(pkg, api, orc):
    abi = pkg.abi
    w, h = 24, 16
    sc, p, origins, dirs, states, want = camera_case(pkg, api, orc, "config3_bvh", w, h, False, None)
    n = 100
    rays = abi.make_path_rays(origins.reshape(-1, 3), dirs.reshape(-1, 3), states.reshape(-1))[:n].copy()
    out = np.zeros(n, dtype=abi.RADIANCE_DTYPE)
    d_rays, d_out = DevBuf(n * 32).upload(rays), DevBuf(n * 16)
    bad, state, ok = abi.RT_ERR_INVALID_ARG, abi.RT_ERR_STATE, abi.RT_OK
    host, dev = api.radiance_trace, api.radiance_trace_buffers
    tr = api.create_tracer(0)
    try:
        tr.set_params(p)  # parameters, no scene
        assert host(tr.h, rays.ctypes.data, n, out.ctypes.data) == state and b"rt_upload_scene" in api.last_error(tr.h)
        assert dev(tr.h, d_rays.ptr, n, d_out.ptr) == state and b"rt_upload_scene" in api.last_error(tr.h)
        tr.close()
        tr = sc.upload(api.create_tracer(0))  # a scene, no parameters
        assert host(tr.h, rays.ctypes.data, n, out.ctypes.data) == state and b"rt_set_params" in api.last_error(tr.h)
        assert dev(tr.h, d_rays.ptr, n, d_out.ptr) == state and b"rt_set_params" in api.last_error(tr.h)
        tr.set_params(p)
        assert host(tr.h, rays.ctypes.data, -1, out.ctypes.data) == bad
        assert host(tr.h, rays.ctypes.data, (1 << 26) + 1, out.ctypes.data) == bad
        assert host(tr.h, None, n, out.ctypes.data) == bad
        assert host(tr.h, rays.ctypes.data, n, None) == bad
        assert host(tr.h, rays.ctypes.data, 2, rays.ctypes.data + 32) == bad  # the output overlaps the rays
        assert host(tr.h, rays.ctypes.data, 0, out.ctypes.data) == ok and host(tr.h, None, 0, None) == ok
        assert dev(tr.h, d_rays.ptr, -1, d_out.ptr) == bad
        assert dev(tr.h, d_rays.ptr, (1 << 26) + 1, d_out.ptr) == bad
        assert dev(tr.h, None, n, d_out.ptr) == bad
        assert dev(tr.h, d_rays.ptr, n, None) == bad
        assert dev(tr.h, rays.ctypes.data, n, d_out.ptr) == bad        # host memory
        assert dev(tr.h, d_rays.ptr, n, out.ctypes.data) == bad
        assert dev(tr.h, d_rays.ptr + 4, n - 1, d_out.ptr) == bad      # misaligned
        assert dev(tr.h, d_rays.ptr, n - 1, d_out.ptr + 4) == bad
        assert dev(tr.h, d_rays.ptr + 32, n, d_out.ptr) == bad         # runs past the allocation
        assert dev(tr.h, d_rays.ptr, n, d_out.ptr + 16) == bad
        assert dev(tr.h, d_rays.ptr, 2, d_rays.ptr + 32) == bad        # the output overlaps the rays
        assert dev(tr.h, d_rays.ptr, 0, d_out.ptr) == ok and dev(tr.h, None, 0, None) == ok
        assert not out.view(np.uint32).any(), "a refused call wrote records"
        assert host(tr.h, rays.ctypes.data, n, out.ctypes.data) == ok
        assert dev(tr.h, d_rays.ptr, n, d_out.ptr) == ok
        tr.synchronize()
        assert_rgb(out["rgb"], want.reshape(-1, 3)[:n], "after the errors")
        assert d_out.download(np.uint8).tobytes() == out.tobytes()
    finally:
        tr.close()
        d_rays.free(), d_out.free()


# ---------------------------------------------------------------- 9. the pass's own watchdog word
def test_watchdog_fails_the_pass_not_the_context(pkg, api, orc, monkeypatch):
    """RT_TRAV_LIMIT=4 (read at rt_upload_scene; the step limit is a software counter, nothing can hang): the walks of the pass are cut
    short.  The host form says so when it returns, the buffer form at the next rt_synchronize or rt_radiance_* call, once — and the
    frames the context rendered before stay readable and equal the oracle's.  Every message names the call that reports and, for a
    deferred report, the call whose pass it was; a pass of another kind (rt_query_occluded) reports its own word only."""
    abi = pkg.abi
    w, h = 24, 16
    sc, p, origins, dirs, states, want = camera_case(pkg, api, orc, "config3_bvh", w, h, False, None)
    rays = abi.make_path_rays(origins.reshape(-1, 3), dirs.reshape(-1, 3), states.reshape(-1))[:256]
    n = len(rays)
    bufs = (DevBuf(n * 32).upload(rays), DevBuf(n * 16))
    images = []
    for lib, tr in ((api, api.create_tracer(0)), (orc, orc.create_tracer(1))):
        try:
            mgr = pkg.scenes.get(3).make_manager(tr, lib, w, h)
            mgr.OnEnable(renderSeed=1)
            mgr.RenderFrames(2)
            images.append(tr.read_accumulated().tobytes())
            if lib is not api:
                continue
            monkeypatch.setenv("RT_TRAV_LIMIT", "4")
            sc.upload(tr)  # the limit of a scene is set when it is uploaded; the images stay
            monkeypatch.delenv("RT_TRAV_LIMIT")

            def reported(e, call, *holds):  # the status, the call at the front of the message, and what else it must hold
                msg = str(e.value)
                assert e.value.status == abi.RT_ERR_HIP and "watchdog" in msg, msg
                assert msg.startswith(f"rt status {abi.RT_ERR_HIP}: {call}: "), msg
                for text in holds:
                    assert text in msg, (text, msg)
                return msg
            family = "in the pass of an rt_radiance_trace_buffers call"
            with pytest.raises(abi.RtError) as e:
                tr.radiance_trace(rays)
            reported(e, "rt_radiance_trace", "in this pass", "the records are not valid")
            tr.radiance_trace_buffers(bufs[0].ptr, n, bufs[1].ptr)  # enqueued: RT_OK
            with pytest.raises(abi.RtError) as e:
                tr.synchronize()
            reported(e, "rt_synchronize", family)
            tr.synchronize()  # reported once
            tr.radiance_trace_buffers(bufs[0].ptr, n, bufs[1].ptr)
            with pytest.raises(abi.RtError) as e:  # the next rt_radiance_* call reports it if it comes first ...
                tr.radiance_trace_buffers(bufs[0].ptr, n, bufs[1].ptr)
            reported(e, "rt_radiance_trace_buffers", family)
            tr.synchronize()  # ... once (and the call that reported enqueued nothing)
            tr.radiance_trace_buffers(bufs[0].ptr, n, bufs[1].ptr)
            with pytest.raises(abi.RtError) as e:  # the host form reports it as well
                tr.radiance_trace(rays)
            reported(e, "rt_radiance_trace", family)
            tr.synchronize()
            # a pass of another kind neither reports it nor is failed by it: a ray query over the same rays says what its own pass
            # met, and the radiance pass is still reported at the next rt_synchronize
            tr.radiance_trace_buffers(bufs[0].ptr, n, bufs[1].ptr)
            with pytest.raises(abi.RtError) as e:
                tr.query_occluded(abi.make_rays(rays["origin"], rays["dir"]))
            assert "rt_radiance" not in reported(e, "rt_query_occluded", "in this pass", "the answers are not valid")
            with pytest.raises(abi.RtError) as e:
                tr.synchronize()
            reported(e, "rt_synchronize", family)
            tr.synchronize()
            assert tr.frame() == 3
            images.append(tr.read_accumulated().tobytes())  # RT_OK: the context's watchdog word was not set
            sc.upload(tr)
            tr.set_params(p)
            assert_rgb(tr.radiance_trace(rays)["rgb"], want.reshape(-1, 3)[:n], "after the re-upload")
        finally:
            tr.close()
    for b in bufs:
        b.free()
    assert images[0] == images[1] == images[2], "the context's frames changed, or differ from the oracle's"
