"""rt_reproject_buffers / rt_reproject_accumulated / rt_resolve* (include/rt_reproject.h) on the GPU.  Every comparison of images is == on
the bit patterns (uint32 views), every pixel, every channel, against the NumPy restatement of the header's prose in
tests/reproject_reference.py (its divide is the oracle's, which tests/test_gpu_math.py pins the device against).

  6. rt_reproject_buffers on synthetic views, 1 x 1 ... 333 x 77, four camera moves; rt_resolve_buffers, also in place;
  7. rt_reproject_accumulated end to end == the restatement applied to what rt_read_accumulated and rt_render_aov returned before the move,
     d_cur_aov_out == rt_render_aov after it; under every RT_LAYOUT, with bound render targets, into torch tensors on a torch stream;
     the whole pipeline on the device: AOVs, reproject, render, resolve, denoise;
  8. geometry: identical views keep the frame count and stay inside their taps, another object / a moved model / glass restart;
  9. frames rendered afterwards == the oracle's frames added onto the reprojected sum;
  10. side effects;  11. errors, the partitioned context, the internal AOV pass's watchdog;  12. it reprojects."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_reference as dref
import reproject_reference as ref
import aov_support as ga
from gpu_support import DevBuf, assert_same_bits
from reproject_support import NEARBY, move_camera, records_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def reproject_on_device(pkg, tr, rgba, prev, cur, p):
    """rt_reproject_buffers on uploaded copies; returns the output and the three inputs as they are afterwards."""
    h, w = rgba.shape[:2]
    bufs = [DevBuf.of(rgba), DevBuf.of(prev), DevBuf.of(cur), DevBuf(rgba.nbytes, fill=0xff)]
    try:
        tr.reproject_buffers(w, h, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, p)
        tr.synchronize()
        return bufs[3].image(h, w), (bufs[0].image(h, w), records_of(pkg, bufs[1], h, w), records_of(pkg, bufs[2], h, w))
    finally:
        for d in bufs:
            d.free()


# ---------------------------------------------------------------- 6. the passes alone, bits
@pytest.mark.parametrize("w,h", [(1, 1), (1, 37), (37, 1), (2, 2), (64, 36), (333, 77)])
def test_reproject_buffers_equals_the_numpy_restatement(pkg, api, orc, w, h):
    tr = api.create_tracer(0)  # no scene, no rt_resize
    try:
        for case in sorted(ref.CAMERAS):
            rgba, prev, cur, cam = ref.synthetic(pkg, w, h, case, seed=w + h)
            for fields in (dict(maxHistory=16.0), dict(flags=1, maxHistory=1000.0, maxPlaneDistance=0.02, minNormalDot=0.99)):
                p = api.reproject_params(prevViewParams=ref.VIEW_PARAMS, prevCamLocalToWorld=cam, **fields)
                got, (rgba2, prev2, cur2) = reproject_on_device(pkg, tr, rgba, prev, cur, p)
                assert rgba2.tobytes() == rgba.tobytes() and prev2.tobytes() == prev.tobytes() and cur2.tobytes() == cur.tobytes(), "an input was written"
                assert_same_bits(got, ref.reproject_with(orc, rgba, prev, cur, p), f"{case} {w} x {h} {fields}")
                if w == 1 or h == 1 or case == "behind":
                    assert not got.view(np.uint32).any(), "a one-pixel-wide or -high image and a camera behind the scene carry nothing"
                elif w > 2:
                    assert (got[..., 3] > 0).mean() > 0.2
    finally:
        tr.close()


def test_the_edges_of_the_previous_image_on_the_device(pkg, api, orc):
    rgba, prev, cur, cam, vp, fx = ref.edge_case(pkg)
    tr = api.create_tracer(0)
    try:
        p = api.reproject_params(prevViewParams=vp, prevCamLocalToWorld=cam, maxPlaneDistance=0.01, maxHistory=100.0)
        got, _ = reproject_on_device(pkg, tr, rgba, prev, cur, p)
        assert_same_bits(got, ref.reproject_with(orc, rgba, prev, cur, p), "edge case")
        assert [bool(got[0, x, 3] > 0) for x in range(len(fx))] == [False, True, True, True, True, True, True, False, False, True]
    finally:
        tr.close()


@pytest.mark.parametrize("w,h", [(1, 1), (37, 21), (333, 77)])
def test_resolve_buffers_equals_the_numpy_restatement_also_in_place(pkg, api, orc, w, h):
    rgba = ref.sums(w, h, w)
    want = ref.resolve(orc, rgba)
    tr = api.create_tracer(0)
    d_in, d_out = DevBuf.of(rgba), DevBuf(rgba.nbytes, fill=0xff)
    try:
        tr.resolve_buffers(w, h, d_in.ptr, d_out.ptr)
        tr.synchronize()
        assert d_in.image(h, w).tobytes() == rgba.tobytes(), "the source image was written"
        assert_same_bits(d_out.image(h, w), want, "resolve")
        tr.resolve_buffers(w, h, d_in.ptr, d_in.ptr)
        tr.synchronize()
        assert_same_bits(d_in.image(h, w), want, "resolve in place")
    finally:
        tr.close()
        d_in.free()
        d_out.free()


# ---------------------------------------------------------------- 7. end to end
E2E = [((3, {}), 80, 45), ("emitters", 64, 36)]


def end_to_end(pkg, api, spec, w, h, frames=5, bound=False, after=0, in_flight=False, **fields):
    """Frames at view A, A's records to the device, view B, rt_reproject_accumulated.  Returns what the calls gave and what the restatement
    needs: (accumulated after, records written to d_cur_aov_out, accumulated before, A's records, B's records by rt_render_aov, params)."""
    tr = api.create_tracer(0)
    n = h * w
    d_prev, d_cur = DevBuf(n * 64, fill=0xff), DevBuf(n * 64, fill=0xff)
    targets = [DevBuf(n * 16), DevBuf(n * 16)] if bound else []
    try:
        su = ga.Setup(pkg, api, tr, spec, w, h)
        if bound:  # (after the manager's rt_resize, which unbinds; the targets are zero, as after rt_reset_accumulation)
            tr.bind_render_targets(targets[0].ptr, targets[1].ptr)
        su.mgr.RenderFrames(frames)
        tr.render_aov_to_device(2, d_prev.ptr, d_prev.nbytes)
        su.mgr.RenderFrames(3)  # in_flight: still running (or held back) in front of the call, which must order itself behind them
        p_a = su.mgr.params()
        before = rec_a = None
        if not in_flight:
            before, rec_a = tr.read_accumulated(), tr.render_aov(2)
            assert records_of(pkg, d_prev, h, w).tobytes() == rec_a.tobytes(), "A's records"
        move_camera(pkg, su.mgr)
        p = api.reproject_params(p_a, **fields)
        tr.reproject_accumulated(p, d_prev.ptr, 3, d_cur.ptr)
        tr.synchronize()
        got = tr.read_accumulated()
        if bound:
            assert targets[1].image(h, w).tobytes() == got.tobytes(), "the bound AccumulatedRender is the one that was reprojected"
        rec_b = tr.render_aov(3)
        extra = None
        if after:
            su.mgr.RenderFrames(after)
            extra = tr.read_accumulated()
        return got, records_of(pkg, d_cur, h, w), before, rec_a, rec_b, p, extra
    finally:
        tr.close()
        for d in [d_prev, d_cur] + targets:
            d.free()


@pytest.mark.parametrize("spec,w,h", E2E, ids=["config3", "emitters"])
def test_reproject_accumulated_equals_numpy_on_the_contexts_own_buffers(pkg, api, orc, spec, w, h, monkeypatch):
    got, cur, before, rec_a, rec_b, p, _ = end_to_end(pkg, api, spec, w, h)
    assert cur.tobytes() == rec_b.tobytes(), "d_cur_aov_out != rt_render_aov at the new view"
    assert rec_a.tobytes() != rec_b.tobytes(), "the camera did not move"
    want = ref.reproject_with(orc, before, rec_a, rec_b, p)
    assert_same_bits(got, want, f"{spec}: rt_reproject_accumulated")
    hit = rec_b["object"] >= 0
    assert (got[..., 3] > 0)[hit].mean() > 0.5 and not got[~hit].view(np.uint32).any()
    assert (got[..., 3][got[..., 3] > 0] <= 8).all()
    for layout in ("dense", "pre,arena,cache"):
        monkeypatch.setenv("RT_LAYOUT", layout)
        other = end_to_end(pkg, api, spec, w, h)
        monkeypatch.delenv("RT_LAYOUT")
        assert_same_bits(other[0], got, f"{spec}: RT_LAYOUT={layout}")
        assert other[1].tobytes() == cur.tobytes()
    for kw in (dict(bound=True), dict(in_flight=True), dict(bound=True, in_flight=True)):
        other = end_to_end(pkg, api, spec, w, h, **kw)
        assert_same_bits(other[0], got, f"{spec}: {kw}")
        assert other[1].tobytes() == cur.tobytes()


_TORCH_CHILD = r"""
import os
import sys
import numpy as np
import torch
torch.cuda.set_device(0)
root = sys.argv[1]
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import __graft_entry__ as graft
import aov_support as ga
import denoise_reference as dref
import reproject_reference as ref
pkg = graft.load_package()
api = pkg.load_library()
orc = graft.load_oracle()
def move(mgr):
    t = mgr.camera.transform
    mgr.camera.transform = pkg.Transform(tuple(np.array(t.position) + np.array((0.25, 0.1, 0.15))), tuple(np.array(t.euler) + np.array((0.0, 2.0, 0.0))))
    mgr.SetShaderParams()
def recs(t, h, w):
    return t.cpu().numpy().view(pkg.abi.AOV_DTYPE).reshape(h, w)
for layout in (None, "dense", "pre,arena,cache"):
    if layout:
        os.environ["RT_LAYOUT"] = layout
    for spec, w, h in (((3, {}), 80, 45), ("emitters", 64, 36)):
        for bound in (False, True):
            tr = api.create_tracer(0)
            s = torch.cuda.Stream()
            tr.set_stream(s.cuda_stream)
            with torch.cuda.stream(s):
                su = ga.Setup(pkg, api, tr, spec, w, h)
                if bound:  # (after the manager's rt_resize, which unbinds)
                    tf = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
                    ta = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
                    s.synchronize()
                    tr.bind_render_targets(tf.data_ptr(), ta.data_ptr())
                su.mgr.RenderFrames(5)
                prev = torch.zeros((h, w, 16), dtype=torch.int32, device="cuda:0")
                cur = torch.zeros((h, w, 16), dtype=torch.int32, device="cuda:0")
                out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
                den = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
                s.synchronize()
                tr.render_aov_to_device(2, prev.data_ptr(), prev.numel() * 4)
                p_a = su.mgr.params()
                before = tr.read_accumulated()
                move(su.mgr)
                p = api.reproject_params(p_a)
                # the whole pipeline without a host copy: reproject, render, resolve, denoise — then one clone on the caller's stream
                tr.reproject_accumulated(p, prev.data_ptr(), 3, cur.data_ptr())
                carried = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0") if not bound else ta.clone()
                su.mgr.RenderFrames(2)
                tr.resolve_to_device(out.data_ptr(), out.numel() * 4)
                tr.denoise_buffers(w, h, out.data_ptr(), cur.data_ptr(), den.data_ptr(), api.denoise_params(scale=1.0))
                first = den.clone()
            s.synchronize()
            tr.synchronize()
            rec_a, rec_b = recs(prev, h, w), recs(cur, h, w)
            want = ref.reproject_with(orc, before, rec_a, rec_b, p)
            if bound:
                assert carried.cpu().numpy().tobytes() == want.tobytes(), "stream order of the reprojection (%s, %s)" % (spec, layout)
            acc = tr.read_accumulated()
            assert (acc[..., 3] >= 2).all() and (acc[..., 3] == want[..., 3] + 2).all(), "two frames onto the carried counts (%s, %s)" % (spec, layout)
            res = ref.resolve(orc, acc)
            assert out.cpu().numpy().tobytes() == res.tobytes() == tr.resolve().tobytes(), "rt_resolve_to_device (%s, %s)" % (spec, layout)
            dp = api.denoise_params(scale=1.0)
            wantd = dref.denoise(orc, res, rec_b, dp.iterations, dp.sigmaColour, dp.sigmaNormal, dp.sigmaPlane, dp.demodulate, dp.scale)
            assert first.cpu().numpy().tobytes() == wantd.tobytes(), "the pipeline's denoised image (%s, %s)" % (spec, layout)
            # rt_reproject_buffers on tensors == the context call
            t_before = torch.from_numpy(before).cuda()
            out2 = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            tr.reproject_buffers(w, h, t_before.data_ptr(), prev.data_ptr(), cur.data_ptr(), out2.data_ptr(), p)
            tr.synchronize()
            assert out2.cpu().numpy().tobytes() == want.tobytes(), "rt_reproject_buffers on tensors (%s, %s)" % (spec, layout)
            tr.set_stream(None)
            tr.synchronize()
            if layout is None and not bound:
                np.save(os.path.join(sys.argv[2], "carried_%dx%d.npy" % (w, h)), want)
            tr.close()
print("REPROJECT_TORCH_OK")
"""


def test_into_torch_tensors_on_a_torch_stream(pkg, api, orc, tmp_path):
    """The calls of the three headers composed on a torch stream given to rt_set_stream, on torch tensors, with own and bound render targets,
    under every RT_LAYOUT: rt_render_aov_to_device, rt_reproject_accumulated, rt_render_frames, rt_resolve_to_device, rt_denoise_buffers — no
    host copy in between, every stage checked against its restatement afterwards.  In a child process that imports torch first, so that the
    library shares torch's HIP runtime."""
    p = subprocess.run([sys.executable, "-c", _TORCH_CHILD, ROOT, str(tmp_path)], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and "REPROJECT_TORCH_OK" in p.stdout, "rc=%d\n%s\n%s" % (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    for spec, w, h in E2E:
        assert (tmp_path / f"carried_{w}x{h}.npy").exists()


# ---------------------------------------------------------------- 8. geometry
def test_identical_views_keep_the_frame_count_and_stay_inside_their_taps(pkg, api, orc):
    """No jitter (divergeStrength = defocusStrength = 0) and the same camera: every hit pixel finds itself.  8 frames: a power of two, so
    that sum_n = 8 * sum_w holds exactly whatever the weights round to, and alpha == min(8, maxHistory) is exact.  A carried mean is a
    convex combination of its taps' means; computed in fp32 (four products, three sums, a divide: each within 2^-24 relative) it may
    leave their range by a few units in the last place, hence 1e-6 relative."""
    w, h, frames = 96, 54, 8
    for max_history in (256.0, 3.0):
        tr = api.create_tracer(0)
        d_prev = DevBuf(h * w * 64)
        try:
            su = ga.Setup(pkg, api, tr, (3, {}), w, h, tweak={"divergeStrength": 0.0, "defocusStrength": 0.0})
            su.mgr.RenderFrames(frames)
            tr.render_aov_to_device(1, d_prev.ptr, d_prev.nbytes)
            before, rec = tr.read_accumulated(), tr.render_aov(1)
            p = api.reproject_params(su.mgr.params(), maxHistory=max_history, flags=1)
            tr.reproject_accumulated(p, d_prev.ptr, 1)
            tr.synchronize()
            got = tr.read_accumulated()
            taps = {}
            assert_same_bits(got, ref.reproject_with(orc, before, rec, rec, p, taps), "identical views")
            hit = rec["object"] >= 0
            assert hit.mean() > 0.2 and (got[..., 3][hit] == min(frames, max_history)).all() and not got[~hit].view(np.uint32).any()
            mean = ref.resolve(orc, got)[..., :3].astype(np.float64)
            src = before[..., :3].astype(np.float64) / before[..., 3:4]
            lo, hi = np.full((h, w, 3), np.inf), np.full((h, w, 3), -np.inf)
            for j in (0, 1):
                for i in (0, 1):
                    qx, qy = taps["x0"] + i, taps["y0"] + j
                    inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                    m = src[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)]
                    lo = np.where(inside[..., None], np.minimum(lo, m), lo)
                    hi = np.where(inside[..., None], np.maximum(hi, m), hi)
            tol = 1e-6 * np.maximum(np.abs(lo), np.abs(hi))
            assert ((mean >= lo - tol) & (mean <= hi + tol))[hit].all()
        finally:
            tr.close()
            d_prev.free()


def test_a_pixel_whose_taps_belong_to_another_object_restarts(pkg, api, orc):
    w, h = 64, 36
    rgba, prev, cur, cam = ref.synthetic(pkg, w, h, "identity", seed=5)
    prev = prev.copy()
    prev["object"][prev["object"] >= 0] += 7
    tr = api.create_tracer(0)
    try:
        p = api.reproject_params(prevViewParams=ref.VIEW_PARAMS, prevCamLocalToWorld=cam, flags=1)
        got, _ = reproject_on_device(pkg, tr, rgba, prev, cur, p)
        assert not got.view(np.uint32).any()
        # one object comes back: exactly its pixels can carry
        prev["object"][prev["object"] == 7] = 0
        got, _ = reproject_on_device(pkg, tr, rgba, prev, cur, p)
        assert (got[..., 3] > 0).any() and not got[cur["object"] != 0].view(np.uint32).any()
    finally:
        tr.close()


def test_a_model_moved_between_the_views_carries_nothing(pkg, api, orc):
    """rt_update_models moves the small model most pixels see, along none of its faces and further than maxPlaneDistance off each; the
    camera stays.  Every pixel that
    now sees the model restarts (the previous view has another object there, or the same one off the tangent plane); the others keep history."""
    w, h = 96, 54
    tr = api.create_tracer(0)
    d_prev = DevBuf(h * w * 64)
    try:
        su = ga.Setup(pkg, api, tr, (3, {}), w, h)
        su.mgr.RenderFrames(4)
        tr.render_aov_to_device(1, d_prev.ptr, d_prev.nbytes)
        before, rec_a, p_a = tr.read_accumulated(), tr.render_aov(1), su.mgr.params()
        ids, counts = np.unique(rec_a["object"][rec_a["object"] >= su.n_spheres], return_counts=True)
        sizes = {int(i): max(su.mgr.models[int(i) - su.n_spheres].transform.scale) for i in ids}  # (the meshes of config 3 are unit cubes)
        small = [(c, int(i)) for i, c in zip(ids, counts) if sizes[int(i)] < 3.0]
        assert small, "no movable model in view"
        target = max(small)[1]
        model = su.mgr.models[target - su.n_spheres]
        t = model.transform
        model.transform = pkg.Transform(tuple(np.array(t.position) + np.array([0.45, 0.35, -0.4])), t.euler, t.scale)
        su.mgr.UpdateModels()
        tr.reproject_accumulated(api.reproject_params(p_a), d_prev.ptr, 1)
        tr.synchronize()
        got, rec_b = tr.read_accumulated(), tr.render_aov(1)
        assert_same_bits(got, ref.reproject_with(orc, before, rec_a, rec_b, api.reproject_params(p_a)), "moved model")
        on_model = rec_b["object"] == target
        assert on_model.sum() > 20 and not got[on_model].view(np.uint32).any()
        others = (rec_b["object"] >= 0) & ~on_model & ((rec_b["hit"] & 3) != 2)
        assert (got[..., 3] > 0)[others].mean() > 0.7
    finally:
        tr.close()
        d_prev.free()


def test_glass_restarts_unless_flag_bit_0_is_set(pkg, api, orc):
    w, h = 72, 40
    out = {}
    for flags in (0, 1):
        tr = api.create_tracer(0)
        d_prev = DevBuf(h * w * 64)
        try:
            su = ga.Setup(pkg, api, tr, "glass_balls_file", w, h)
            su.mgr.RenderFrames(4)
            tr.render_aov_to_device(1, d_prev.ptr, d_prev.nbytes)
            before, rec, p_a = tr.read_accumulated(), tr.render_aov(1), su.mgr.params()
            move_camera(pkg, su.mgr, offset=(0.05, 0.0, 0.0), turn=(0, 0, 0))
            p = api.reproject_params(p_a, flags=flags)
            tr.reproject_accumulated(p, d_prev.ptr, 1)
            tr.synchronize()
            got, rec_b = tr.read_accumulated(), tr.render_aov(1)
            assert_same_bits(got, ref.reproject_with(orc, before, rec, rec_b, p), f"glass, flags {flags}")
            out[flags] = (got, (rec_b["hit"] & 3) == 2, (rec_b["hit"] & 3) == 1)
        finally:
            tr.close()
            d_prev.free()
    (g0, glass, opaque), (g1, _, _) = out[0], out[1]
    assert glass.sum() > 20 and opaque.sum() > 20
    assert not g0[glass].view(np.uint32).any() and (g1[..., 3][glass] > 0).mean() > 0.5
    assert g0[opaque].tobytes() == g1[opaque].tobytes() and (g0[..., 3][opaque] > 0).mean() > 0.5


# ---------------------------------------------------------------- 9. accumulation afterwards
@pytest.mark.parametrize("k", [1, 19])
def test_frames_rendered_afterwards_add_onto_the_reprojected_sum_like_the_oracles(pkg, api, orc, k):
    """K frames after the reprojection == the oracle's K frames (same Frame values, same view) added in frame order onto the reprojected sum,
    all four components: the trace kernels add float4(col, 1) onto whatever the accumulator holds.  19 frames: a fused launch and more."""
    spec, w, h, frames = (3, {}), 64, 36, 5
    got, _, _, _, _, _, extra = end_to_end(pkg, api, spec, w, h, frames=frames, after=k)
    ot = orc.create_tracer(16)
    try:
        so = ga.Setup(pkg, orc, ot, spec, w, h)
        so.mgr.RenderFrames(frames + 3)  # (end_to_end renders 3 more frames at A before it moves)
        move_camera(pkg, so.mgr)
        ot.write_accumulated(got)
        so.mgr.RenderFrames(k)
        want = ot.read_accumulated()
    finally:
        ot.close()
    assert_same_bits(extra, want, f"{k} frames onto the reprojected sum")
    assert (extra[..., 3] == got[..., 3] + k).all()


# ---------------------------------------------------------------- 10. side effects
def test_side_effects_are_the_documented_ones(pkg, api):
    w, h = 96, 54
    tr = api.create_tracer(0)
    tr.enable_stats(True)
    n = h * w
    d_prev, d_cur, t, t2 = DevBuf(n * 64), DevBuf(n * 64), DevBuf(n * 16), DevBuf(n * 16)
    try:
        su = ga.Setup(pkg, api, tr, (3, {}), w, h, seed=5)
        su.mgr.RenderFrames(17)
        for _ in range(3):
            su.mgr.RenderFrame()  # rt_render_frame may hold these back
        tr.render_aov_to_device(1, d_prev.ptr, d_prev.nbytes)
        p = api.reproject_params(su.mgr.params())

        def state():
            c = tr.counters()
            c.pop("gpuMs")
            return tr.frame(), c, tr.read_frame().tobytes()
        s0, acc0 = state(), tr.read_accumulated()
        # the calls that change nothing at all
        tr.reproject_buffers(w, h, tr.render_targets()[1], d_prev.ptr, d_prev.ptr, t.ptr, p)
        tr.resolve_buffers(w, h, t.ptr, t2.ptr)
        tr.resolve_to_device(t2.ptr, t2.nbytes)
        res = tr.resolve()
        tr.synchronize()
        assert t2.image(h, w).tobytes() == res.tobytes()
        assert state() == s0 and tr.read_accumulated().tobytes() == acc0.tobytes()
        # the call that changes AccumulatedRender and nothing else
        move_camera(pkg, su.mgr)
        s1 = state()
        assert s1 == s0
        tr.reproject_accumulated(p, d_prev.ptr, 1, d_cur.ptr)
        tr.synchronize()
        assert state() == s1
        assert tr.read_accumulated().tobytes() != acc0.tobytes()
        su.mgr.RenderFrames(2)
        assert tr.frame() == s0[0] + 2
    finally:
        tr.close()
        for d in (d_prev, d_cur, t, t2):
            d.free()


def test_a_set_watchdog_word_stays_as_it_is(pkg, api, monkeypatch):
    """Frames rendered under RT_TRAV_LIMIT=4 (the hook of tests/test_gpu_watchdog.py) set the context's watchdog word: every host read fails
    with a message that holds the word's value.  The calls of this header leave that message exactly as it was — rt_write_accumulated
    would have cleared it; rt_resolve, a host read, fails like the others."""
    w, h = 64, 36
    tr = api.create_tracer(0)
    n = h * w
    d_prev, t, t2 = DevBuf(n * 64), DevBuf(n * 16), DevBuf(n * 16)
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
        tr.reproject_accumulated(p, d_prev.ptr, 1)  # (its own AOV pass is cut short too: reported by the synchronise, once)
        with pytest.raises(pkg.abi.RtError):
            tr.synchronize()
        tr.reproject_buffers(w, h, t.ptr, d_prev.ptr, d_prev.ptr, t2.ptr, p)
        tr.resolve_buffers(w, h, t.ptr, t2.ptr)
        tr.resolve_to_device(t2.ptr, t2.nbytes)
        tr.synchronize()
        with pytest.raises(pkg.abi.RtError) as e:
            tr.resolve()
        assert "fired" in str(e.value)
        assert word() == before and tr.frame() == 3
    finally:
        tr.close()
        for d in (d_prev, t, t2):
            d.free()


# ---------------------------------------------------------------- 11. errors
def test_errors(pkg, api):
    abi = pkg.abi
    w, h = 64, 36
    img = np.zeros((h, w, 4), dtype=F)
    d_in, d_out, d_prev, d_cur = DevBuf(img.nbytes), DevBuf(img.nbytes), DevBuf(h * w * 64), DevBuf(h * w * 64)
    ok = api.reproject_params(prevViewParams=ref.VIEW_PARAMS, prevCamLocalToWorld=ref.camera())
    tr = api.create_tracer(0)

    def buffers(p=ok, ww=w, hh=h, a=None, b=None, c=None, d=None):
        return api.reproject_buffers(tr.h, C.byref(p) if p is not None else None, ww, hh, d_in.ptr if a is None else a, d_prev.ptr if b is None else b,
                                     d_cur.ptr if c is None else c, d_out.ptr if d is None else d)

    def accumulated(p=ok, prev=None, frame=1, cur=-1):
        return api.reproject_accumulated(tr.h, C.byref(p) if p is not None else None, d_prev.ptr if prev is None else prev, frame, d_cur.ptr if cur == -1 else cur)

    def resolves(nbytes=img.nbytes):
        return api.resolve(tr.h, img.ctypes.data, nbytes), api.resolve_to_device(tr.h, d_out.ptr, nbytes)
    try:
        # the context calls need an image (and rt_reproject_accumulated a scene and parameters); the *_buffers calls need none of them
        assert accumulated() == abi.RT_ERR_STATE and resolves() == (abi.RT_ERR_STATE,) * 2  # before rt_resize
        assert buffers() == abi.RT_OK and api.resolve_buffers(tr.h, w, h, d_in.ptr, d_out.ptr) == abi.RT_OK
        tr.resize(w, h)
        assert accumulated() == abi.RT_ERR_STATE  # before rt_upload_scene
        assert resolves() == (abi.RT_OK,) * 2
        mgr = ga.scene_of(pkg, (3, {})).make_manager(tr, api, w, h)
        mgr.InitTexturesAndBuffers()
        mgr.InitBVH()
        assert accumulated() == abi.RT_ERR_STATE  # before rt_set_params
        tr.close()
        tr = api.create_tracer(0)
        ga.Setup(pkg, api, tr, (3, {}), w, h)
        for fields in (dict(maxPlaneDistance=-0.5), dict(maxPlaneDistance=float("nan")), dict(maxPlaneDistance=float("inf")), dict(minNormalDot=float("nan")),
                       dict(minNormalDot=float("-inf")), dict(maxHistory=0.0), dict(maxHistory=-1.0), dict(maxHistory=float("inf")), dict(maxHistory=float("nan")),
                       dict(flags=2), dict(flags=0x80000001), dict(reserved=1)):
            p = api.reproject_params(**fields)
            assert buffers(p) == abi.RT_ERR_INVALID_ARG, fields
            assert accumulated(p) == abi.RT_ERR_INVALID_ARG, fields
        assert buffers(None) == abi.RT_ERR_INVALID_ARG and accumulated(None) == abi.RT_ERR_INVALID_ARG
        for size in (0, 96, 104):
            p = api.reproject_params(struct_size=size)
            assert buffers(p) == abi.RT_ERR_ABI_MISMATCH and accumulated(p) == abi.RT_ERR_ABI_MISMATCH
        assert buffers(api.reproject_params(maxPlaneDistance=0.0, minNormalDot=-2.0, flags=1)) == abi.RT_OK
        # sizes and pointers
        assert buffers(ww=0) == abi.RT_ERR_INVALID_ARG and buffers(hh=0) == abi.RT_ERR_INVALID_ARG and buffers(ww=-4) == abi.RT_ERR_INVALID_ARG
        assert buffers(ww=1 << 16, hh=1 << 15) == abi.RT_ERR_INVALID_ARG
        for which in "abcd":
            assert buffers(**{which: 0}) == abi.RT_ERR_INVALID_ARG  # null
            assert buffers(**{which: d_in.ptr + 4}) == abi.RT_ERR_INVALID_ARG  # misaligned
            assert buffers(**{which: img.ctypes.data}) == abi.RT_ERR_INVALID_ARG  # host memory
        assert buffers(a=d_in.ptr + 16) == abi.RT_ERR_INVALID_ARG and buffers(b=d_prev.ptr + 64) == abi.RT_ERR_INVALID_ARG  # run past the allocation
        assert buffers(d=d_in.ptr) == abi.RT_ERR_INVALID_ARG  # out == in
        assert buffers(hh=h // 2, d=d_prev.ptr + 16) == abi.RT_ERR_INVALID_ARG and buffers(hh=h // 2, d=d_cur.ptr + 16) == abi.RT_ERR_INVALID_ARG
        assert buffers(hh=h // 2, d=d_in.ptr + (h // 4) * w * 16) == abi.RT_ERR_INVALID_ARG  # out overlaps in
        assert buffers(hh=h // 2, d=d_in.ptr + (h // 2) * w * 16) == abi.RT_OK  # adjacent halves of one allocation do not
        assert buffers(c=d_prev.ptr) == abi.RT_OK  # inputs may be the same memory
        rb = lambda a, b, ww=w, hh=h: api.resolve_buffers(tr.h, ww, hh, a, b)
        assert rb(d_in.ptr, d_in.ptr) == abi.RT_OK  # in place
        assert rb(d_in.ptr, d_in.ptr + 16, hh=h // 2) == abi.RT_ERR_INVALID_ARG  # partial overlap
        assert rb(d_in.ptr, d_in.ptr + (h // 2) * w * 16, hh=h // 2) == abi.RT_OK
        for bad in (0, d_in.ptr + 4, img.ctypes.data):
            assert rb(bad, d_out.ptr) == abi.RT_ERR_INVALID_ARG and rb(d_in.ptr, bad) == abi.RT_ERR_INVALID_ARG
        assert rb(d_in.ptr, d_out.ptr, ww=0) == abi.RT_ERR_INVALID_ARG and rb(d_in.ptr, d_out.ptr + 16) == abi.RT_ERR_INVALID_ARG
        assert accumulated(frame=0) == abi.RT_ERR_INVALID_ARG and accumulated(frame=-2) == abi.RT_ERR_INVALID_ARG
        for bad in (0, d_prev.ptr + 4, d_prev.ptr + 64, img.ctypes.data):
            assert accumulated(prev=bad) == abi.RT_ERR_INVALID_ARG
        for bad in (d_cur.ptr + 4, d_cur.ptr + 64, img.ctypes.data, d_prev.ptr):
            assert accumulated(cur=bad) == abi.RT_ERR_INVALID_ARG
        frame_ptr, accum_ptr = tr.render_targets()
        assert accumulated(prev=accum_ptr) == abi.RT_ERR_INVALID_ARG and accumulated(cur=accum_ptr) == abi.RT_ERR_INVALID_ARG
        assert resolves(img.nbytes - 16) == (abi.RT_ERR_INVALID_ARG,) * 2 and resolves(img.nbytes + 16) == (abi.RT_ERR_INVALID_ARG,) * 2
        assert api.resolve(tr.h, None, img.nbytes) == abi.RT_ERR_INVALID_ARG and api.resolve_to_device(tr.h, None, img.nbytes) == abi.RT_ERR_INVALID_ARG
        for bad in (img.ctypes.data, d_out.ptr + 4, d_out.ptr + 16, accum_ptr):
            assert api.resolve_to_device(tr.h, bad, img.nbytes) == abi.RT_ERR_INVALID_ARG
        assert accumulated() == abi.RT_OK and accumulated(cur=None) == abi.RT_OK and resolves() == (abi.RT_OK,) * 2 and buffers() == abi.RT_OK
        tr.synchronize()
        tr.close()
        # a context that owns part of the image
        tr = api.create_tracer(0)
        tr.set_partition(8, 0, 2)
        ga.Setup(pkg, api, tr, (3, {}), w, h)
        rows = tr.local_rows()
        assert 0 < rows < h
        assert accumulated() == abi.RT_ERR_STATE and buffers() == abi.RT_ERR_STATE
        assert b"part" in api.last_error(tr.h)
        assert resolves(rows * w * 16) == (abi.RT_OK,) * 2  # a per-pixel divide: its own rows
        tr.set_partition(8, 0, 1)  # the whole image again
        assert accumulated() == abi.RT_OK
        tr.synchronize()
        mt = api.create_multi_tracer([0, 0])
        try:
            for call in (mt.reproject_accumulated, mt.resolve, mt.resolve_to_device):
                with pytest.raises(abi.RtError) as e:
                    call()
                assert e.value.status == abi.RT_ERR_STATE
        finally:
            mt.close()
    finally:
        tr.close()
        for d in (d_in, d_out, d_prev, d_cur):
            d.free()


def test_watchdog_of_the_internal_aov_pass_leaves_the_accumulator_untouched(pkg, api, monkeypatch):
    """RT_TRAV_LIMIT=4 (read at rt_upload_scene; the step limit is a software counter, nothing can hang): the internal pass's walks are cut
    short.  rt_reproject_accumulated enqueues and returns RT_OK; the next rt_synchronize reports the pass's watchdog, once; and the
    accumulator — a checkpoint written with rt_write_accumulated — holds exactly the bytes it held."""
    w, h = 64, 36
    tr = api.create_tracer(0)
    d_prev, d_cur = DevBuf(h * w * 64), DevBuf(h * w * 64)
    try:
        monkeypatch.setenv("RT_TRAV_LIMIT", "4")
        su = ga.Setup(pkg, api, tr, (3, {}), w, h)
        monkeypatch.delenv("RT_TRAV_LIMIT")
        image = ref.sums(w, h, 11)
        tr.write_accumulated(image)
        p = api.reproject_params(su.mgr.params())
        tr.reproject_accumulated(p, d_prev.ptr, 1, d_cur.ptr)  # enqueued: RT_OK
        with pytest.raises(pkg.abi.RtError) as e:
            tr.synchronize()
        assert e.value.status == pkg.abi.RT_ERR_HIP and "watchdog" in str(e.value), str(e.value)
        tr.synchronize()  # reported once
        assert tr.read_accumulated().tobytes() == image.tobytes()
        assert tr.counters()["segments"] == 0 and tr.frame() == 1
        # rt_resolve, a host read that comes before any rt_synchronize, reports it too — once — and does not hand out a resolve of the
        # untouched accumulator as if it were the reprojected image
        tr.reproject_accumulated(p, d_prev.ptr, 1)
        with pytest.raises(pkg.abi.RtError) as e:
            tr.resolve()
        assert e.value.status == pkg.abi.RT_ERR_HIP and "watchdog" in str(e.value) and "rt_reproject_accumulated" in str(e.value), str(e.value)
        tr.synchronize()
        assert tr.read_accumulated().tobytes() == image.tobytes()
        finite = np.isfinite(image).all(axis=-1) & (image[..., 3] > 0)
        assert np.array_equal(tr.resolve()[..., 3].view(np.uint32), image[..., 3].view(np.uint32)) and finite.any()
    finally:
        tr.close()
        d_prev.free()
        d_cur.free()


# ---------------------------------------------------------------- 12. it reprojects
def test_it_reprojects(pkg, api):
    """Config 3 at 320 x 180.  32 frames at view A, a move to the nearby view B, rt_reproject_accumulated with the default parameters, 4 more
    frames, rt_resolve: C.  R: reset at B, then 4 frames.  G: the mean of 1,024 frames at B.  Over the pixels with carried history,
    mse(C, G) < 0.5 * mse(R, G), and those pixels are more than half of the hit pixels.  Variance ~ 1 / n predicts 4 / 36 = 0.11 on
    diffuse surfaces; the factor above that is room for bilinear blur and view-dependent shading.

    "Nearby": the camera of config 3 stands 5.7 units from the scene's centre; B is 0.06 units (1 % of that) and 0.4 degrees away — what an
    interactive camera covers between two displayed frames, the use this call is for.

    Measured on an MI355X with the defaults (maxPlaneDistance 0.1, minNormalDot 0.9, maxHistory 256), the only set tried:
    carried 55,469 of 57,600 hit pixels, mse(32 carried + 4) = 0.0557, mse(reset + 4) = 0.1683, ratio 0.331
    (profiles/r08_reproject.txt, which also has the CPU values of the oracle's images through the restatement at 96 x 54 and 192 x 108 —
    0.45 ... 0.77 for moves up to twice this one, above 1 for a move five times as large — and why: tools/reproject_cpu_check.py)."""
    w, h = 320, 180

    def run(frames_a, frames_b, reproject):
        tr = api.create_tracer(0)
        d_prev = DevBuf(h * w * 64)
        try:
            su = ga.Setup(pkg, api, tr, (3, {}), w, h)
            carried = None
            if frames_a:
                su.mgr.RenderFrames(frames_a)
                tr.render_aov_to_device(1, d_prev.ptr, d_prev.nbytes)
            p_a = su.mgr.params()
            move_camera(pkg, su.mgr, **NEARBY)
            if reproject:
                tr.reproject_accumulated(api.reproject_params(p_a), d_prev.ptr, 1)
                carried = tr.read_accumulated()[..., 3] > 0
            su.mgr.RenderFrames(frames_b)
            return tr.resolve()[..., :3].astype(np.float64), carried, tr.render_aov(1)
        finally:
            tr.close()
            d_prev.free()
    truth, _, aov = run(0, 1024, False)
    reset, _, _ = run(0, 4, False)
    moved, carried, _ = run(32, 4, True)
    hit = aov["object"] >= 0
    mse_c = float(((moved - truth)[carried] ** 2).mean())
    mse_r = float(((reset - truth)[carried] ** 2).mean())
    print(f"rt_reproject defaults: carried {int(carried.sum())} of {int(hit.sum())} hit pixels ({carried.sum() / hit.sum():.4f}); "
          f"mse(32 carried + 4, truth) = {mse_c:.6g}, mse(reset + 4, truth) = {mse_r:.6g}, ratio = {mse_c / mse_r:.4f}")
    assert carried.sum() > 0.5 * hit.sum()
    assert np.isfinite(mse_c) and mse_c < 0.5 * mse_r
