"""rt_query_closest / rt_query_occluded and their *_buffers forms (include/rt_query.h) on the GPU: caller-made rays against the uploaded
scene.  Every comparison is == on the bit patterns (uint32 views: NaN and -0 count), every ray, every field.

  1. closest hit == oracle_ray_collision, all ten values, and == rt_debug_intersect on the same rays;
  2. `object` in range with the material flag the oracle's hit carries; `triangle` -1 exactly where no model was hit, inside its model's
     range, and for identity-transform models oracle_ray_triangle on it returns the record's dst;
  3. occlusion == (didHit && d < tmax) from the oracle's d, for tmax in {+inf, d, the two neighbours of d, d / 2, 0, -1, NaN};
  4. block and grid edges: n = 0, 1, 63, 64, 65, 130 are prefixes of a larger batch; RT_GRID=2 with more blocks than waves; guard words
     behind the outputs;
  5. the buffer forms (DevBuf, and torch tensors in a child process), stream order behind rt_update_spheres and held-back frames;
  6. no visible state change, on a context that was never resized and on a strip partition;
  7. RT_LAYOUT does not change the records;  8. every row of the header's error list;  9. the pass's own watchdog word.

Scenes — the smallest that reach each kernel variant: config 2 (FLAT: spheres + quads), config 3 (BVH), 70 models + 5 spheres (MANY;
two of the models untransformed, for rule 2), glass_balls (the glass class).  About 2,000 rays per scene from a fixed seed (make_rays
in tests/query_support.py); the oracle's records are computed once per scene and shared."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from flush_table import held_at
from gpu_support import DevBuf, bits
from query_support import SCENES, assert_same_records, case, records_from_oracle, snapshot

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
F3 = C.c_float * 3


@pytest.fixture()
def tracer(api):
    tr = api.create_tracer(0)
    yield tr
    tr.close()


# ---------------------------------------------------------------- 1 + 2. the closest hit
@pytest.mark.parametrize("name", SCENES)
def test_closest_hit_equals_the_oracle_and_the_debug_hook(pkg, api, orc, tracer, name):
    sc, origins, dirs, want10 = case(pkg, api, orc, name)
    abi = pkg.abi
    n = len(origins)
    hit = want10[:, 0] != 0
    print(f"{name}: {n} rays, {int(hit.sum())} hit, {int((~hit).sum())} miss")
    assert hit.sum() >= n // 4 and (~hit).sum() >= n // 4, "the generator must give at least a quarter hits and a quarter misses"
    sc.upload(tracer)  # never resized, no parameters
    got = tracer.query_closest(abi.make_rays(origins, dirs, tmax=-1.0))  # (tmax plays no part)
    assert got.dtype == abi.RAYHIT_DTYPE and got.shape == (n,)
    # the oracle's misses carry zeros beside dst = +inf, as the header states for the record
    assert np.isposinf(want10[~hit, 2]).all() and not want10[~hit][:, [0, 1, 3, 4, 5, 6, 7, 8, 9]].any()
    assert_same_records(got, records_from_oracle(pkg, sc, want10, got["object"], got["triangle"]), name)
    assert not got["reserved"].any()
    # pos as the oracle formed it: origin + dir * dst, one rounding per operation
    with np.errstate(all="ignore"):
        pos = origins[hit] + dirs[hit] * want10[hit, 2:3]
    assert bits(pos).tolist() == bits(got["pos"][hit]).tolist()
    # rule 2: object and triangle
    obj = got["object"]
    assert ((obj >= 0) == hit).all() and (obj < len(sc.materials)).all()
    assert (sc.materials["flag"][obj[hit]].astype(F) == want10[hit, 9]).all(), "material flag of the record's object != the oracle's hit"
    is_model = obj >= sc.n_spheres
    assert ((got["triangle"] >= 0) == is_model).all(), "triangle is -1 exactly where no model was hit"
    identity = np.eye(4, dtype=F).T.reshape(16)
    out6 = (C.c_float * 6)()
    checked = 0
    for i in np.argwhere(is_model).ravel():
        mi, t = int(obj[i]) - sc.n_spheres, int(got["triangle"][i])
        off = int(sc.models["triOffset"][mi])
        assert off <= t < off + int(sc.tri_count[mi]), (i, mi, t, off)
        if np.array_equal(sc.models["localToWorld"][mi], identity) and np.array_equal(sc.models["worldToLocal"][mi], identity):
            cull = int(sc.models["material"]["flag"][mi]) != 2  # RC:355
            orc.ray_triangle(F3(*origins[i]), F3(*dirs[i]), sc.triangles[t:t + 1].ctypes.data, int(cull), out6)
            assert out6[0] != 0, (i, "the reported triangle is not hit by the ray")
            assert bits(np.array([out6[2]], dtype=F))[0] == bits(got["dst"][i:i + 1])[0], (i, out6[2], got["dst"][i])
            checked += 1
    # the shared fields == rt_debug_intersect on the same rays
    dbg = tracer.debug_intersect(origins, dirs)
    assert bits(dbg[:, 2]).tolist() == bits(got["dst"]).tolist()
    assert np.array_equal(dbg[:, 0] != 0, (got["hit"] & 3) != 0) and np.array_equal(dbg[:, 1] != 0, (got["hit"] & 0x100) != 0)
    assert bits(dbg[:, 3:6]).tolist() == bits(got["normal"]).tolist() and bits(dbg[:, 6:9]).tolist() == bits(got["pos"]).tolist()
    assert np.array_equal(dbg[hit, 9] == abi.MATERIAL_GLASS, (got["hit"][hit] & 3) == 2)
    # the case covers what it is there for
    backface = (got["hit"] & 0x100) != 0
    assert backface.any() and (hit & ~backface).any()
    assert (obj[hit] < sc.n_spheres).any() or sc.n_spheres == 0
    if name == "config2_flat":
        assert is_model.any() and (obj[hit] < sc.n_spheres).any()
    if name == "crowded70_many":
        assert checked > 0, "no identity-transform model was hit"
        assert (obj >= sc.n_spheres + 64).any(), "no hit on a model beyond the 64-bit mask"
    if name == "glass_balls":
        assert ((got["hit"] & 3) == 2).any() and ((got["hit"] & 3) == 1).any()


# ---------------------------------------------------------------- 3. occlusion
@pytest.mark.parametrize("name", SCENES)
def test_occlusion_equals_the_contract(pkg, api, orc, tracer, name):
    sc, origins, dirs, want10 = case(pkg, api, orc, name)
    abi = pkg.abi
    hit = want10[:, 0] != 0
    d = np.where(hit, want10[:, 2], F(1)).astype(F)
    sc.upload(tracer)
    with np.errstate(all="ignore"):
        tmaxes = [("+inf", np.full_like(d, np.inf)), ("d", d), ("next above d", np.nextafter(d, F(np.inf))), ("next below d", np.nextafter(d, F(-np.inf))),
                  ("d / 2", d / F(2)), ("0", np.zeros_like(d)), ("-1", np.full_like(d, -1)), ("NaN", np.full_like(d, np.nan))]
        for what, tmax in tmaxes:
            tmax = tmax.astype(F)
            got = tracer.query_occluded(abi.make_rays(origins, dirs, tmax=tmax))
            assert got.dtype == np.uint32 and set(got.tolist()) <= {0, 1}
            want = (hit & (want10[:, 2] < tmax)).astype(np.uint32)
            bad = np.argwhere(got != want).ravel()
            assert not len(bad), f"{name}, tmax = {what}: {len(bad)} rays differ; first is ray {bad[0]}: got {got[bad[0]]}, d = {want10[bad[0], 2]}, tmax = {tmax[bad[0]]}"
            if what == "+inf":
                assert np.array_equal(got != 0, tracer.query_closest(abi.make_rays(origins, dirs))["object"] >= 0)
                assert got.any() and not got.all()
            if what in ("d", "next below d", "0", "-1", "NaN"):
                assert not got.any()
            if what == "next above d":
                assert np.array_equal(got != 0, hit)


# ---------------------------------------------------------------- 4. block and grid edges
@pytest.mark.parametrize("name", ["config2_flat", "config3_bvh", "crowded70_many"])
def test_batch_sizes_are_prefixes_and_nothing_is_written_behind_the_last_record(pkg, api, orc, name):
    sc, origins, dirs, want10 = case(pkg, api, orc, name)
    abi = pkg.abi
    tr = sc.upload(api.create_tracer(0))
    guard = 64
    try:
        # in a fixed shuffled order (the generator's groups come one after the other), tmax on either side of the hit distance
        perm = np.random.default_rng(1).permutation(len(origins))
        tmax = np.where(want10[:, 0] != 0, want10[:, 2] * np.where(np.arange(len(origins)) % 2 == 0, F(1.5), F(0.5)), F(1)).astype(F)
        rays = abi.make_rays(origins, dirs, tmax=tmax)[perm]
        full_hits, full_occ = tr.query_closest(rays[:400]), tr.query_occluded(rays[:400])
        assert full_occ.any() and not full_occ.all() and (full_hits["object"][full_occ == 0] >= 0).any()
        d_rays = DevBuf(400 * 32).upload(rays[:400])
        for n in (0, 1, 63, 64, 65, 130):
            hits, occ = tr.query_closest(rays[:n]), tr.query_occluded(rays[:n])
            assert hits.shape == (n,) and occ.shape == (n,)
            assert hits.tobytes() == full_hits[:n].tobytes() and occ.tobytes() == full_occ[:n].tobytes(), n
            # the buffer forms, with guard words behind the outputs
            d_hits, d_occ = DevBuf(n * 48 + guard, fill=0xa5), DevBuf(n * 4 + guard, fill=0xa5)
            tr.query_closest_buffers(d_rays.ptr if n else None, n, d_hits.ptr if n else None)
            tr.query_occluded_buffers(d_rays.ptr if n else None, n, d_occ.ptr if n else None)
            tr.synchronize()
            raw_hits, raw_occ = d_hits.download(np.uint8), d_occ.download(np.uint8)
            assert raw_hits[:n * 48].tobytes() == full_hits[:n].tobytes() and (raw_hits[n * 48:] == 0xa5).all(), n
            assert raw_occ[:n * 4].tobytes() == full_occ[:n].tobytes() and (raw_occ[n * 4:] == 0xa5).all(), n
            d_hits.free(), d_occ.free()
        d_rays.free()
    finally:
        tr.close()


@pytest.mark.parametrize("name", ["config2_flat", "config3_bvh"])
def test_a_grid_of_two_waves_goes_round_more_than_once(pkg, api, orc, name, monkeypatch):
    sc, origins, dirs, want10 = case(pkg, api, orc, name)
    n = 64 * 5 + 3
    rays = pkg.abi.make_rays(origins[:n], dirs[:n], tmax=np.where(want10[:n, 0] != 0, want10[:n, 2] * F(1.5), F(1)).astype(F))
    out = []
    for grid in (None, "2"):
        if grid:
            monkeypatch.setenv("RT_GRID", grid)  # read at rt_create
        tr = api.create_tracer(0)
        monkeypatch.delenv("RT_GRID", raising=False)
        try:
            sc.upload(tr)
            out.append((tr.query_closest(rays).tobytes(), tr.query_occluded(rays).tobytes()))
        finally:
            tr.close()
    assert out[0] == out[1]
    assert np.frombuffer(out[0][1], dtype=np.uint32).any()


# ---------------------------------------------------------------- 5. forms
def test_buffer_forms_see_updates_and_run_behind_held_back_frames(pkg, api, orc, forced=False):
    """A query enqueued right behind rt_update_spheres sees the moved sphere; queries between rt_render_frame calls that are held back
    leave the image what the same frames give without any query."""
    abi = pkg.abi
    w, h = 64, 36
    images = []
    for with_queries in (True, False):
        tr = api.create_tracer(0)
        try:
            mgr = pkg.scenes.get(2).make_manager(tr, api, w, h)
            mgr.OnEnable(renderSeed=3)
            spheres = mgr._pack_spheres()
            c, r = spheres["centre"][0].astype(np.float64), float(spheres["radius"][0])
            # a ray that grazes past sphere 0 where it stands and meets it head on once it has moved by 3 radii along x
            moved = c + [3 * r, 0, 0]
            ray = abi.make_rays([moved + [0, 0, -50 * r]], [[0, 0, 1]])
            ray = np.repeat(ray, 70)
            d_rays, d_hits, d_occ = DevBuf(ray.nbytes).upload(ray), DevBuf(70 * 48), DevBuf(70 * 4)
            if with_queries:
                before = tr.query_closest(ray)
                assert (before["object"] != 0).all()
            mgr.RenderFrames(5)
            for _ in range(3):  # rt_render_frame may hold these back
                mgr.RenderFrame()
                if with_queries:
                    held_at(tr, "test_gpu_query: rt_query_closest_buffers behind rt_render_frame", forced)
                    tr.query_closest_buffers(d_rays.ptr, 70, d_hits.ptr)
                    tr.query_occluded_buffers(d_rays.ptr, 70, d_occ.ptr)
            if with_queries:
                spheres["centre"][0] = moved
                tr.update_spheres(spheres)
                tr.query_closest_buffers(d_rays.ptr, 70, d_hits.ptr)  # no synchronise in between
                tr.query_occluded_buffers(d_rays.ptr, 70, d_occ.ptr)
                tr.synchronize()
                hits = d_hits.download(abi.RAYHIT_DTYPE)
                assert (hits["object"] == 0).all() and (d_occ.download(np.uint32) == 1).all()
                assert_same_records(hits, tr.query_closest(ray), "buffer form vs host form")
                assert abs(float(hits["dst"][0]) - 49 * r) < 1e-3 * r
                spheres["centre"][0] = c
                tr.update_spheres(spheres)  # back, for the frames that follow
            mgr.RenderFrames(4)
            images.append((tr.read_accumulated().tobytes(), tr.read_frame().tobytes(), tr.frame()))
            for b in (d_rays, d_hits, d_occ):
                b.free()
        finally:
            tr.close()
    assert images[0] == images[1]


def test_buffer_forms_run_behind_frames_that_are_held_back_for_certain(pkg, api, orc, monkeypatch):
    """The same with RT_HOLD_BACK=1: every rt_render_frame of the burst IS held back (asserted right before each pass)."""
    monkeypatch.setenv("RT_HOLD_BACK", "1")
    test_buffer_forms_see_updates_and_run_behind_held_back_frames(pkg, api, orc, forced=True)


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
    mgr.InitBVH()  # the scene alone
    n = 1000
    o = rng.normal(size=(n, 3)); o = 12 * o / np.linalg.norm(o, axis=1, keepdims=True) + [0, 1, 0]
    d = rng.uniform(-2, 2, (n, 3)) + [0, 1, 0] - o
    rays = abi.make_rays(o, d, tmax=rng.uniform(0.5, 1.5, n).astype(np.float32))
    host_hits, host_occ = tr.query_closest(rays), tr.query_occluded(rays)
    assert (host_hits["object"] >= 0).any() and (host_hits["object"] < 0).any() and host_occ.any() and not host_occ.all()
    t_rays = torch.from_numpy(rays.view(np.float32).reshape(n, 8).copy()).to("cuda:0")
    t_hits = torch.full((n, 12), 0x7fc00001, dtype=torch.int32, device="cuda:0")
    t_occ = torch.full((n,), 7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    tr.query_closest_buffers(t_rays.data_ptr(), n, t_hits.data_ptr())
    tr.query_occluded_buffers(t_rays.data_ptr(), n, t_occ.data_ptr())
    tr.synchronize()
    assert t_hits.cpu().numpy().tobytes() == host_hits.tobytes(), "tensor != host form (config %d)" % cfg
    assert t_occ.cpu().numpy().view(np.uint32).tolist() == host_occ.tolist(), "occlusion tensor != host form (config %d)" % cfg
    # on the caller's stream (rt_set_stream): work enqueued on that stream behind the pass sees its answers
    s = torch.cuda.Stream()
    tr.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        t2 = torch.zeros((n,), dtype=torch.int32, device="cuda:0")
        s.synchronize()
        tr.query_occluded_buffers(t_rays.data_ptr(), n, t2.data_ptr())
        total = t2.sum()
    s.synchronize()
    assert int(total.item()) == int(host_occ.sum()), "stream order (config %d)" % cfg
    tr.set_stream(None)
    tr.synchronize()
    tr.close()
print("QUERY_TORCH_OK")
"""


def test_buffer_forms_into_torch_tensors(pkg, api):
    """rt_query_*_buffers on torch tensors' data_ptr()s == the host forms, and in the order of a torch stream given to rt_set_stream.
    In a child process that imports torch first, so that the library shares torch's HIP runtime."""
    p = subprocess.run([sys.executable, "-c", _TORCH_CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "QUERY_TORCH_OK" in p.stdout, "rc=%d\n%s\n%s" % (p.returncode, p.stdout[-3000:], p.stderr[-3000:])


# ---------------------------------------------------------------- 6. no visible state change
def mixed_calls(tr, rays, bufs):
    d_rays, d_hits, d_occ = bufs
    n = len(rays)
    hits, occ = tr.query_closest(rays), tr.query_occluded(rays)
    tr.query_closest_buffers(d_rays.ptr, n, d_hits.ptr)
    tr.query_occluded_buffers(d_rays.ptr, n, d_occ.ptr)
    tr.synchronize()
    assert d_hits.download(np.uint8).tobytes() == hits.tobytes() and d_occ.download(np.uint32).tolist() == occ.tolist()
    return hits, occ


def test_query_calls_leave_no_trace(pkg, api, orc):
    sc, origins, dirs, want10 = case(pkg, api, orc, "config3_bvh")
    abi = pkg.abi
    n = 500
    rays = abi.make_rays(origins[:n], dirs[:n], tmax=np.where(want10[:n, 0] != 0, want10[:n, 2] * F(1.5), F(1)).astype(F))
    bufs = (DevBuf(n * 32).upload(rays), DevBuf(n * 48), DevBuf(n * 4))
    w, h = 64, 40
    try:
        # a context that was never resized answers, and its state reads as before
        tr = sc.upload(api.create_tracer(0))
        whole = mixed_calls(tr, rays, bufs)
        assert tr.frame() == 1
        tr.close()
        assert_same_records(whole[0], records_from_oracle(pkg, sc, want10[:n], whole[0]["object"], whole[0]["triangle"]), "never resized")
        # a rendering context, whole and as part 1 of 2 of a strip partition: everything a caller can read is the same before and after
        for part in (None, 1):
            tr = api.create_tracer(0)
            tr.enable_stats(True)
            if part is not None:
                tr.set_partition(8, part, 2)
            mgr = pkg.scenes.get(3).make_manager(tr, api, w, h)
            mgr.OnEnable(renderSeed=5)
            mgr.RenderFrames(4)
            tr.variance_update()
            mgr.RenderFrames(4)
            tr.variance_update()
            tr.adaptive_select(tr.adaptive_params(threshold=0.01, minFrames=0))
            mgr.RenderFrame()
            before = snapshot(tr)
            got = mixed_calls(tr, rays, bufs)
            mgr_frames = tr.frame()
            after = snapshot(tr)
            assert before == after, [k for k in before if before[k] != after[k]]
            assert mgr_frames == before["frame"]
            assert_same_records(got[0], whole[0], f"partition {part}")
            assert got[1].tolist() == whole[1].tolist()
            tr.close()
    finally:
        for b in bufs:
            b.free()


# ---------------------------------------------------------------- 7. layouts
def test_device_layout_does_not_change_the_records(pkg, api, orc, monkeypatch):
    sc, origins, dirs, want10 = case(pkg, api, orc, "config3_bvh")
    rays = pkg.abi.make_rays(origins, dirs, tmax=np.where(want10[:, 0] != 0, want10[:, 2] * F(1.5), F(1)).astype(F))
    out = []
    for layout in ("dense", "pre,arena,cache"):  # the layouts tests/test_gpu_cost_view.py cycles through
        monkeypatch.setenv("RT_LAYOUT", layout)  # read by rt_upload_scene
        tr = api.create_tracer(0)
        try:
            sc.upload(tr)
            monkeypatch.delenv("RT_LAYOUT")
            out.append((tr.query_closest(rays), tr.query_occluded(rays)))
        finally:
            tr.close()
    assert_same_records(out[0][0], out[1][0], "RT_LAYOUT dense vs pre,arena,cache")
    assert out[0][1].tolist() == out[1][1].tolist()
    assert (out[0][0]["triangle"] >= 0).any()


# ---------------------------------------------------------------- 8. errors
def test_errors(pkg, api, orc):
    abi = pkg.abi
    sc, origins, dirs, _ = case(pkg, api, orc, "config3_bvh")
    n = 100
    rays = abi.make_rays(origins[:n], dirs[:n])
    hits, occ = np.zeros(n, dtype=abi.RAYHIT_DTYPE), np.zeros(n, dtype=np.uint32)
    d_rays, d_hits, d_occ = DevBuf(n * 32).upload(rays), DevBuf(n * 48), DevBuf(n * 4)
    host = ((api.query_closest, hits.ctypes.data), (api.query_occluded, occ.ctypes.data))
    dev = ((api.query_closest_buffers, d_hits.ptr, 48), (api.query_occluded_buffers, d_occ.ptr, 4))
    bad, state, ok = abi.RT_ERR_INVALID_ARG, abi.RT_ERR_STATE, abi.RT_OK
    tr = api.create_tracer(0)
    try:
        for call, out in host:
            assert call(tr.h, rays.ctypes.data, n, out) == state  # before rt_upload_scene
            assert b"rt_upload_scene" in api.last_error(tr.h)
        for call, out, _ in dev:
            assert call(tr.h, d_rays.ptr, n, out) == state
        sc.upload(tr)
        for call, out in host:
            assert call(tr.h, rays.ctypes.data, -1, out) == bad
            assert call(tr.h, rays.ctypes.data, (1 << 26) + 1, out) == bad
            assert call(tr.h, None, n, out) == bad
            assert call(tr.h, rays.ctypes.data, n, None) == bad
            assert call(tr.h, rays.ctypes.data, 2, rays.ctypes.data + 32) == bad  # the output overlaps the rays
            assert call(tr.h, rays.ctypes.data, 0, out) == ok and call(tr.h, None, 0, None) == ok
        for call, out, per in dev:
            assert call(tr.h, d_rays.ptr, -1, out) == bad
            assert call(tr.h, d_rays.ptr, (1 << 26) + 1, out) == bad
            assert call(tr.h, None, n, out) == bad
            assert call(tr.h, d_rays.ptr, n, None) == bad
            assert call(tr.h, rays.ctypes.data, n, out) == bad        # host memory
            assert call(tr.h, d_rays.ptr, n, hits.ctypes.data) == bad
            assert call(tr.h, d_rays.ptr + 4, n - 1, out) == bad      # misaligned
            assert call(tr.h, d_rays.ptr, n - 1, out + 4) == bad
            assert call(tr.h, d_rays.ptr + 32, n, out) == bad         # runs past the allocation
            assert call(tr.h, d_rays.ptr, n, out + 16) == bad
            assert call(tr.h, d_rays.ptr, 2, d_rays.ptr + 32) == bad  # the output overlaps the rays
            assert call(tr.h, d_rays.ptr, 0, out) == ok and call(tr.h, None, 0, None) == ok
        for call, out in host:
            assert call(tr.h, rays.ctypes.data, n, out) == ok
        for call, out, _ in dev:
            assert call(tr.h, d_rays.ptr, n, out) == ok
        tr.synchronize()
        assert (hits["object"] >= 0).any() and d_hits.download(np.uint8).tobytes() == hits.tobytes()
        assert d_occ.download(np.uint32).tolist() == occ.tolist()
    finally:
        tr.close()
        for b in (d_rays, d_hits, d_occ):
            b.free()


# ---------------------------------------------------------------- 9. the pass's own watchdog word
def test_watchdog_fails_the_pass_not_the_context(pkg, api, orc, monkeypatch):
    """RT_TRAV_LIMIT=4 (read at rt_upload_scene; the step limit is a software counter, nothing can hang): the walks are cut short.  The
    host forms say so when they return, a buffer form at the next rt_synchronize, once — and the context's counters and images, which
    no frame of it touched, stay readable.  After a re-upload without the variable the same rays equal the oracle again.  Every message
    names the call that reports and, for a deferred report, the calls whose pass it was; the next rt_query_* call reports in place of
    rt_synchronize when it comes first; a pass of another kind (rt_render_aov) reports its own word only."""
    sc, origins, dirs, want10 = case(pkg, api, orc, "config3_bvh")
    abi = pkg.abi
    n = 256
    rays = abi.make_rays(origins[:n], dirs[:n])
    bufs = (DevBuf(n * 32).upload(rays), DevBuf(n * 48), DevBuf(n * 4))
    tr = api.create_tracer(0)
    try:
        mgr = pkg.scenes.get(3).make_manager(tr, api, 64, 36)
        monkeypatch.setenv("RT_TRAV_LIMIT", "4")
        mgr.OnEnable(renderSeed=1)  # resize, upload, parameters; no frame
        monkeypatch.delenv("RT_TRAV_LIMIT")

        def reported(e, call, *holds):  # the status, the call at the front of the message, and what else it must hold
            msg = str(e.value)
            assert e.value.status == abi.RT_ERR_HIP and "watchdog" in msg, msg
            assert msg.startswith(f"rt status {abi.RT_ERR_HIP}: {call}: "), msg
            for text in holds:
                assert text in msg, (text, msg)
            return msg
        family = "in the pass of an rt_query_closest_buffers or rt_query_occluded_buffers call"
        for call, name, noun in ((tr.query_closest, "rt_query_closest", "records"), (tr.query_occluded, "rt_query_occluded", "answers")):
            with pytest.raises(abi.RtError) as e:
                call(rays)
            reported(e, name, "in this pass", f"the {noun} are not valid")
        tr.query_closest_buffers(bufs[0].ptr, n, bufs[1].ptr)  # enqueued: RT_OK
        with pytest.raises(abi.RtError) as e:
            tr.synchronize()
        reported(e, "rt_synchronize", family)
        tr.synchronize()  # reported once
        tr.query_closest_buffers(bufs[0].ptr, n, bufs[1].ptr)
        with pytest.raises(abi.RtError) as e:  # the next rt_query_* call reports it if it comes first ...
            tr.query_occluded_buffers(bufs[0].ptr, n, bufs[2].ptr)
        reported(e, "rt_query_occluded_buffers", family)
        tr.synchronize()  # ... once (and the call that reported enqueued nothing)
        tr.query_occluded_buffers(bufs[0].ptr, n, bufs[2].ptr)
        with pytest.raises(abi.RtError) as e:  # a host form reports it as well
            tr.query_closest(rays)
        reported(e, "rt_query_closest", family)
        tr.synchronize()
        # a pass of another kind neither reports it nor is failed by it: rt_render_aov says what its own pass met, and the query pass
        # is still reported at the next rt_synchronize
        tr.query_closest_buffers(bufs[0].ptr, n, bufs[1].ptr)
        with pytest.raises(abi.RtError) as e:
            tr.render_aov(1)
        assert "rt_query" not in reported(e, "rt_render_aov", "a kernel watchdog fired")
        with pytest.raises(abi.RtError) as e:
            tr.synchronize()
        reported(e, "rt_synchronize", family)
        tr.synchronize()
        c = tr.counters()  # RT_OK: the context's watchdog word was not set
        assert c["segments"] == 0
        assert not tr.read_accumulated().any()
        assert tr.frame() == 1
        sc.upload(tr)  # the limit of a scene is set when it is uploaded
        got = tr.query_closest(rays)
        assert_same_records(got, records_from_oracle(pkg, sc, want10[:n], got["object"], got["triangle"]), "after the re-upload")
    finally:
        tr.close()
        for b in bufs:
            b.free()
