"""rt_render_aov / rt_render_aov_to_device (include/rt_aov.h) on the GPU: what camera ray 0 of a frame hits first, per pixel.
Every comparison is == on the bit patterns (uint32 views: NaN and -0 count), every pixel, every field.

  4. anchor without restated ray maths: in a scene of emitters (emissionStrength 1, distinct dyadic colours), no sky, no bounce, one
     ray per pixel, the oracle's rendered frame N IS the emission of what camera ray 0 hit (RC:485-538, 530-531 with a transmittance
     of exactly 1) — so aov.emission == the oracle's frame, and aov.object names that palette entry;
  5. every field against the oracle's functions: the test restates RCC:15 + RC:550-576 in fp32, one rounding per operation, with the
     draws from oracle_next_random / oracle_random_point_in_circle and the divide / normalise from oracle_math_eval, and feeds each
     ray to oracle_ray_collision, oracle_material_colour and oracle_environment_light; the restated rays are held by 4 and by
     HIP rt_debug_intersect on them == the AOV records;
  6. `triangle`: inside its model's range, and for identity-transform models oracle_ray_triangle on it returns the record's dst;
  7. hit class == rt_render_cost's firstHit;
  8. the same records under every device layout, strip partition, for 1 x N and N x 1 images, and through the device variant into a
     torch tensor;
  9. no visible state change;  10. errors, and the pass's own watchdog word (RT_TRAV_LIMIT, the hook tests/test_gpu_watchdog.py uses)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from aov_support import Setup, assert_records_equal, camera_rays, check_triangles, emitter_scene, oracle_records, scene_of
from flush_table import held_at
from gpu_support import DevBuf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ---------------------------------------------------------------- RCC:15 + RC:550-576 restated (the test's own arithmetic)
def gpu_aov(pkg, api, spec, w, h, frame, tweak=None, seed=1):
    tr = api.create_tracer(0)
    try:
        Setup(pkg, api, tr, spec, w, h, tweak, seed)
        return tr.render_aov(frame)
    finally:
        tr.close()


# ---------------------------------------------------------------- 4. the anchor
def oracle_emitter_frame(pkg, orc, spec, w, h, frame, seed=1):
    ot = orc.create_tracer(8)
    try:
        su = Setup(pkg, orc, ot, spec, w, h, seed=seed)
        su.mgr.RenderFrames(frame)
        return ot.read_frame()[..., :3].copy()  # the frame rendered last: frame `frame`
    finally:
        ot.close()


def palette_index(img, palette):
    """Per pixel: the palette entry whose colour the pixel has exactly, -1 for (0, 0, 0); fails on any other colour."""
    idx = np.full(img.shape[:2], -2, dtype=np.int64)
    idx[(img.view(np.uint32) == 0).all(axis=-1)] = -1
    for k, col in enumerate(palette):
        idx[(img.view(np.uint32) == np.array(col, dtype=F).view(np.uint32)).all(axis=-1)] = k
    assert (idx != -2).all(), f"{int((idx == -2).sum())} pixels are neither a palette colour nor black"
    return idx


@pytest.mark.parametrize("spec", ["emitters", "emitters_dof"])
@pytest.mark.parametrize("frame", [1, 2, 17])
def test_emission_is_the_oracles_frame_of_an_emitter_scene(pkg, api, orc, spec, frame):
    w, h = 64, 36
    palette = emitter_scene(pkg, 0.0)[1]
    want = oracle_emitter_frame(pkg, orc, spec, w, h, frame)
    which = palette_index(want, palette)  # the oracle alone: only palette colours and black, and both occur
    assert (which == -1).any() and len(set(which[which >= 0].tolist())) >= 8, sorted(set(which.ravel().tolist()))
    aov = gpu_aov(pkg, api, spec, w, h, frame)
    assert aov["emission"].view(np.uint32).tolist() == want.view(np.uint32).tolist()
    # object -> palette entry: spheres carry palette[0..2], model i carries palette[3 + i]
    assert np.array_equal(aov["object"], which)
    assert np.array_equal((aov["hit"] & 3) != 0, which >= 0)


# ---------------------------------------------------------------- 5 + 6 + 7. every field, every pixel
FIELD_CASES = [  # name, scene, W, H, frame, tweaks
    ("config2_flat", (2, {}), 64, 36, 1, {}),
    ("config2_flat_f5_nosky", (2, {}), 64, 36, 5, {"useSky": False}),
    ("config3_bvh", (3, {}), 64, 36, 1, {}),
    ("config3_bvh_f9", (3, {}), 48, 27, 9, {}),
    ("glass_balls", "glass_balls_file", 72, 40, 2, {}),
    ("crowded70_many", "crowded70", 64, 36, 3, {}),
    ("config4_dof", (4, {"subdivisions": 3}), 64, 36, 1, {}),
    ("emitters_identity_models", "emitters", 64, 36, 4, {"useSky": True}),
]


@pytest.mark.parametrize("case", FIELD_CASES, ids=[c[0] for c in FIELD_CASES])
def test_every_field_of_every_pixel_equals_the_oracles_functions(pkg, api, orc, case):
    name, spec, w, h, frame, tweak = case
    tr, ot = api.create_tracer(0), orc.create_tracer(1)
    try:
        su = Setup(pkg, api, tr, spec, w, h, tweak)
        so = Setup(pkg, orc, ot, spec, w, h, tweak)
        p = su.params(frame)
        aov = tr.render_aov(frame)
        assert aov.shape == (h, w) and aov.dtype == pkg.abi.AOV_DTYPE
        origins, dirs = camera_rays(orc, p, w, h, frame)
        want = oracle_records(pkg, orc, ot, so, p, origins, dirs, aov["object"])
        want["triangle"] = aov["triangle"]  # (rule 6 below)
        assert_records_equal(aov, want, name)
        hit = aov["hit"] & 3
        assert np.array_equal(aov["object"] >= 0, hit != 0)
        # the restated rays themselves: HIP's own intersection of them is the record
        dbg = tr.debug_intersect(origins.reshape(-1, 3), dirs.reshape(-1, 3)).reshape(h, w, 10)
        assert dbg[..., 2].view(np.uint32).tolist() == aov["dst"].view(np.uint32).tolist()
        assert np.array_equal(dbg[..., 0] != 0, hit != 0) and np.array_equal(dbg[..., 1] != 0, (aov["hit"] & 0x100) != 0)
        assert dbg[..., 3:6].view(np.uint32).tolist() == aov["normal"].view(np.uint32).tolist()
        assert dbg[..., 6:9].view(np.uint32).tolist() == aov["pos"].view(np.uint32).tolist()
        # rule 6
        n_tri = check_triangles(orc, so, aov, origins, dirs)
        # rule 7
        cost = tr.render_cost(frame)
        assert np.array_equal(hit, cost[..., 7])
        # the case covers what it is there for
        if spec == (2, {}):
            checker = su.materials["flag"] == pkg.abi.MATERIAL_CHECKERED
            assert checker.any() and checker[aov["object"][hit != 0]].any(), "no checker-flag material in view"
            assert (hit == 0).any() and (aov["object"][hit != 0] < su.n_spheres).any()
        if spec == "glass_balls_file":
            assert (hit == 2).any() and (hit == 1).any()
        if spec == "emitters":
            assert n_tri > 0, "no identity-transform model in view"
        if tweak.get("useSky", su.mgr.useSky) and (hit == 0).any():
            assert aov["albedo"][hit == 0].any()
    finally:
        tr.close()
        ot.close()


# ---------------------------------------------------------------- 8. invariance
def test_device_layout_does_not_change_the_records(pkg, api, monkeypatch):
    out = []
    for layout in ("dense", "pre,arena,cache"):  # the layouts tests/test_gpu_cost_view.py cycles through
        monkeypatch.setenv("RT_LAYOUT", layout)
        out.append(gpu_aov(pkg, api, (3, {}), 96, 54, 3))
        monkeypatch.delenv("RT_LAYOUT")
    assert_records_equal(out[0], out[1], "RT_LAYOUT dense vs pre,arena,cache")
    assert (out[0]["triangle"] >= 0).any()


@pytest.mark.parametrize("spec", [(3, {}), (2, {})], ids=["bvh", "flat"])
@pytest.mark.parametrize("strip_rows", [8, 136])
def test_strip_partitions_reassemble_the_image(pkg, api, spec, strip_rows):
    w, h, frame, parts = 40, 300, 2, 3
    full = gpu_aov(pkg, api, spec, w, h, frame)
    whole = np.zeros_like(full)
    seen = np.zeros(h, dtype=int)
    for i in range(parts):
        tr = api.create_tracer(0)
        try:
            tr.set_partition(strip_rows, i, parts)
            Setup(pkg, api, tr, spec, w, h)
            local = tr.render_aov(frame)
            rows = tr.local_to_global_rows()
            assert local.shape == (len(rows), w)
            whole[rows] = local
            seen[rows] += 1
        finally:
            tr.close()
    assert (seen == 1).all()
    assert_records_equal(whole, full, f"strip_rows {strip_rows}, {parts} parts")
    if strip_rows == 8:
        mt = api.create_multi_tracer([0, 0, 0])
        try:
            Setup(pkg, api, mt, spec, w, h)
            assert_records_equal(mt.render_aov(frame), full, "MultiTracer.render_aov")
        finally:
            mt.close()


@pytest.mark.parametrize("w,h", [(1, 37), (37, 1)])
def test_one_pixel_wide_and_high_images(pkg, api, orc, w, h):
    """uv = 0 / 0 in one direction: every pixel shoots a NaN ray from the camera origin; the record is what rt_debug_intersect gives for it."""
    tr = api.create_tracer(0)
    try:
        su = Setup(pkg, api, tr, (3, {}), w, h)
        aov = tr.render_aov(1)
        origins, dirs = camera_rays(orc, su.params(1), w, h, 1)
        assert np.isnan(dirs).all() and np.isfinite(origins).all()
        dbg = tr.debug_intersect(origins.reshape(-1, 3), dirs.reshape(-1, 3)).reshape(h, w, 10)
        assert dbg[..., 2].view(np.uint32).tolist() == aov["dst"].view(np.uint32).tolist()
        assert np.array_equal(dbg[..., 0] != 0, (aov["hit"] & 3) != 0)
        assert dbg[..., 3:6].view(np.uint32).tolist() == aov["normal"].view(np.uint32).tolist()
        assert dbg[..., 6:9].view(np.uint32).tolist() == aov["pos"].view(np.uint32).tolist()
    finally:
        tr.close()


def test_device_variant_equals_the_host_variant(pkg, api):
    w, h, frame = 96, 54, 3
    for spec in ((3, {}), (2, {}), "crowded70"):
        tr = api.create_tracer(0)
        d = DevBuf(h * w * 64, fill=0xff)
        try:
            su = Setup(pkg, api, tr, spec, w, h)
            host = tr.render_aov(frame)
            su.mgr.RenderFrames(3)  # frames in flight in front of the pass
            tr.render_aov_to_device(frame, d.ptr, d.nbytes)
            tr.synchronize()
            assert_records_equal(d.records(pkg, h, w), host, f"rt_render_aov_to_device vs rt_render_aov ({spec})")
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
w, h, frame = 96, 54, 3
for cfg in (3, 2):
    tr = api.create_tracer(0)
    mgr = pkg.scenes.get(cfg).make_manager(tr, api, w, h)
    mgr.OnEnable(renderSeed=1)
    host = tr.render_aov(frame)
    mgr.RenderFrames(3)
    t = torch.full((h, w, 16), 0x7fc00001, dtype=torch.int32, device="cuda:0")
    tr.render_aov_to_device(frame, t.data_ptr(), t.numel() * 4)
    tr.synchronize()
    dev = t.cpu().numpy().view(pkg.abi.AOV_DTYPE).reshape(h, w)
    assert dev.tobytes() == host.tobytes(), "tensor != host variant (config %d)" % cfg
    # on the caller's stream (rt_set_stream): work enqueued on that stream behind the pass sees its records
    s = torch.cuda.Stream()
    tr.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        t2 = torch.zeros((h, w, 16), dtype=torch.int32, device="cuda:0")
        s.synchronize()
        tr.render_aov_to_device(frame, t2.data_ptr(), t2.numel() * 4)
        first = t2[..., 0].clone()
    s.synchronize()
    assert first.cpu().numpy().view(np.uint32).tolist() == host["dst"].view(np.uint32).tolist(), "stream order (config %d)" % cfg
    tr.set_stream(None)
    tr.synchronize()
    tr.close()
print("AOV_TORCH_OK")
"""


def test_device_variant_into_a_torch_tensor(pkg, api):
    """rt_render_aov_to_device(frame, tensor.data_ptr(), ...) == rt_render_aov, and in the order of a torch stream given to
    rt_set_stream.  In a child process that imports torch first, so that the library shares torch's HIP runtime."""
    p = subprocess.run([sys.executable, "-c", _TORCH_CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "AOV_TORCH_OK" in p.stdout, "rc=%d\n%s\n%s" % (p.returncode, p.stdout[-3000:], p.stderr[-3000:])


# ---------------------------------------------------------------- 9. no visible state change
def test_aov_calls_leave_no_trace(pkg, api, orc, forced=False):
    cfg, w, h, seed = (3, {}), 96, 54, 5
    snaps, seen = [], {}
    for with_aov in (True, False):
        tr = api.create_tracer(0)
        tr.enable_stats(True)
        su = Setup(pkg, api, tr, cfg, w, h, seed=seed)
        mgr = su.mgr
        t = DevBuf(h * w * 64)

        def probe(tag):
            if with_aov:
                if tag.startswith("after held"):    # (rt_get_counters below launches held frames too: this pass comes first)
                    held_at(tr, "test_gpu_aov: rt_render_aov after held-back frames", forced)
                    met = tr.render_aov(tr.frame())
                before = (tr.frame(), tr.counters())
                a = tr.render_aov(tr.frame())  # the frame the context renders next
                assert_records_equal(a, tr.render_aov(tr.frame()), tag)
                if tag.startswith("after held"):
                    assert_records_equal(a, met, tag)
                tr.render_aov_to_device(1, t.ptr, t.nbytes)
                first = tr.render_aov(1)
                assert_records_equal(first, seen.setdefault(1, first), tag)
                after = (tr.frame(), tr.counters())
                before[1].pop("gpuMs"), after[1].pop("gpuMs")
                assert before == after, tag
        mgr.RenderFrame()                       # frame 1
        probe("after rt_render_frame")
        mgr.RenderFrames(17)                    # frames 2-18: a fused launch, still running when the pass comes
        probe("after rt_render_frames(17)")
        for _ in range(3):                      # frames 19-21: rt_render_frame may hold them back (pending)
            mgr.RenderFrame()
        probe("after held-back frames")
        mgr.RenderFrames(14)                    # frames 22-35, the second of two rt_render_frames calls around a pass
        probe("after the second rt_render_frames")
        c = tr.counters()
        c.pop("gpuMs")
        snaps.append((tr.read_accumulated(), tr.read_frame(), tr.frame(), c))  # (the reads succeed: the watchdog word is clear)
        tr.close()
        t.free()
    (acc_a, frame_a, n_a, c_a), (acc_b, frame_b, n_b, c_b) = snaps
    assert acc_a.tobytes() == acc_b.tobytes() and frame_a.tobytes() == frame_b.tobytes()
    assert n_a == n_b == 36 and c_a == c_b
    ot = orc.create_tracer(16)
    Setup(pkg, orc, ot, cfg, w, h, seed=seed).mgr.RenderFrames(35)
    acc_o = ot.read_accumulated()
    ot.close()
    assert acc_a.view(np.uint32).tobytes() == acc_o.view(np.uint32).tobytes(), "accumulated image != oracle"


def test_aov_calls_leave_no_trace_with_frames_held_back_for_certain(pkg, api, orc, monkeypatch):
    """The same with RT_HOLD_BACK=1: frames 19-21 ARE held back when the AOV pass comes (asserted right before it)."""
    monkeypatch.setenv("RT_HOLD_BACK", "1")
    test_aov_calls_leave_no_trace(pkg, api, orc, forced=True)


# ---------------------------------------------------------------- 10. errors, and the pass's own watchdog word
def test_errors(pkg, api):
    abi = pkg.abi
    buf = np.zeros((36, 64), dtype=abi.AOV_DTYPE)
    dev = DevBuf(buf.nbytes)
    calls = ((api.render_aov, buf.ctypes.data), (api.render_aov_to_device, dev.ptr))
    tr = api.create_tracer(0)
    try:
        for call, ptr in calls:
            assert call(tr.h, 1, ptr, buf.nbytes) == abi.RT_ERR_STATE  # before rt_resize
        tr.resize(64, 36)
        for call, ptr in calls:
            assert call(tr.h, 1, ptr, buf.nbytes) == abi.RT_ERR_STATE  # before rt_upload_scene
        Setup(pkg, api, tr, (3, {}), 64, 36)
        for call, ptr in calls:
            assert call(tr.h, 1, ptr, buf.nbytes - 64) == abi.RT_ERR_INVALID_ARG
            assert call(tr.h, 1, ptr, buf.nbytes + 64) == abi.RT_ERR_INVALID_ARG
            assert call(tr.h, 1, None, buf.nbytes) == abi.RT_ERR_INVALID_ARG
            assert call(tr.h, 0, ptr, buf.nbytes) == abi.RT_ERR_INVALID_ARG
            assert call(tr.h, -3, ptr, buf.nbytes) == abi.RT_ERR_INVALID_ARG
        # the device variant writes through its pointer: host memory, a misaligned pointer and too small an allocation are refused
        assert api.render_aov_to_device(tr.h, 1, buf.ctypes.data, buf.nbytes) == abi.RT_ERR_INVALID_ARG
        assert api.render_aov_to_device(tr.h, 1, dev.ptr + 4, buf.nbytes) == abi.RT_ERR_INVALID_ARG
        assert api.render_aov_to_device(tr.h, 1, dev.ptr + 64, buf.nbytes) == abi.RT_ERR_INVALID_ARG  # runs past the allocation
        for call, ptr in calls:
            assert call(tr.h, 1, ptr, buf.nbytes) == abi.RT_OK
        tr.synchronize()
        assert (buf["hit"] & 3).any()
        assert_records_equal(dev.records(pkg, 36, 64), buf, "device vs host")
    finally:
        tr.close()
    tr = api.create_tracer(0)
    try:
        tr.resize(64, 36)
        mgr = scene_of(pkg, (3, {})).make_manager(tr, api, 64, 36)
        mgr.InitTexturesAndBuffers()
        mgr.InitBVH()  # a scene, but no rt_set_params yet
        for call, ptr in calls:
            assert call(tr.h, 1, ptr, buf.nbytes) == abi.RT_ERR_STATE
    finally:
        tr.close()
        dev.free()


def test_watchdog_fails_the_pass_not_the_context(pkg, api, monkeypatch):
    """RT_TRAV_LIMIT=4 (read at rt_upload_scene; the step limit is a software counter, nothing can hang): the pass's walks are cut short.
    The host variant says so when it returns, the device variant at the next rt_synchronize, once — and the context's counters and
    images, which no frame of it touched, stay readable.  Every message names the call that reports and, for a deferred report, the
    calls whose pass it was; the next AOV call reports in place of rt_synchronize when it comes first; a pass of another kind
    (rt_query_closest) reports its own word only."""
    tr = api.create_tracer(0)
    t = DevBuf(36 * 64 * 64)
    try:
        monkeypatch.setenv("RT_TRAV_LIMIT", "4")
        su = Setup(pkg, api, tr, (3, {}), 64, 36)
        monkeypatch.delenv("RT_TRAV_LIMIT")
        abi = pkg.abi

        def reported(e, call, *holds):  # the status, the call at the front of the message, and what else it must hold
            msg = str(e.value)
            assert e.value.status == abi.RT_ERR_HIP and "watchdog" in msg, msg
            assert msg.startswith(f"rt status {abi.RT_ERR_HIP}: {call}: "), msg
            for text in holds:
                assert text in msg, (text, msg)
            return msg
        family = "in the AOV pass of an rt_render_aov_to_device, rt_denoise_to_device or rt_reproject_accumulated call"
        for call, name in ((lambda: tr.render_aov(1), "rt_render_aov"), (tr.render_aov_centre, "rt_render_aov_centre")):
            with pytest.raises(abi.RtError) as e:
                call()
            reported(e, name, "a kernel watchdog fired")
        tr.render_aov_to_device(1, t.ptr, t.nbytes)  # enqueued: RT_OK
        with pytest.raises(abi.RtError) as e:
            tr.synchronize()
        reported(e, "rt_synchronize", family)
        tr.synchronize()  # reported once
        tr.render_aov_to_device(1, t.ptr, t.nbytes)
        with pytest.raises(abi.RtError) as e:  # the next AOV call reports it if it comes first ...
            tr.render_aov_to_device(1, t.ptr, t.nbytes)
        reported(e, "rt_render_aov_to_device", family)
        tr.synchronize()  # ... once (and the call that reported enqueued nothing)
        tr.render_aov_to_device(1, t.ptr, t.nbytes)
        with pytest.raises(abi.RtError) as e:  # the host variant reports it as well
            tr.render_aov(1)
        reported(e, "rt_render_aov", family)
        tr.synchronize()
        # a pass of another kind neither reports it nor is failed by it: a ray query along the camera's axis says what its own pass met,
        # and the AOV pass is still reported at the next rt_synchronize
        m = np.array(list(su.params(1).camLocalToWorld), dtype=F)
        rays = abi.make_rays(np.tile(m[12:15], (64, 1)), np.tile(m[8:11], (64, 1)))
        tr.render_aov_to_device(1, t.ptr, t.nbytes)
        with pytest.raises(abi.RtError) as e:
            tr.query_closest(rays)
        assert "AOV" not in reported(e, "rt_query_closest", "in this pass", "the records are not valid")
        with pytest.raises(abi.RtError) as e:
            tr.synchronize()
        reported(e, "rt_synchronize", family)
        tr.synchronize()
        c = tr.counters()  # RT_OK: the context's watchdog word was not set
        assert c["segments"] == 0
        assert not tr.read_accumulated().any()
        assert tr.frame() == 1
    finally:
        tr.close()
        t.free()
