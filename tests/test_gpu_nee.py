"""rt_nee_trace / rt_nee_trace_buffers / rt_nee_light_count (include/rt_nee.h) on the GPU.

  1. bit for bit, rgb and rng, against tests/nee_reference.py (the header's estimator restated path by path over rt_query_closest, the
     oracle's draws and functions, and a numpy light table): 200 camera rays and their prefixes n = 1, 63, 64, 65, maxBounceCount -1, 0,
     1 and the scene's own, on seven scenes — FLAT (three spheres, two emissive, a quad light), config 3 (triangle emitters through a
     BVH), the 70-model scene with a model and a sphere made emissive (MANY), a quad light under a mirroring transform, a glass sphere
     between light and floor, a camera inside an emissive sphere, and the instances of item 8 — and with a grid of two waves;
  2. the two identities: every scene with its emitters stripped, and an all-mirror scene with emitters, give rt_radiance_trace's bits;
  3. physics in closed form: the radiance a diffuse floor reflects under one spherical emitter, for NEE and for plain radiance, and the
     ratio of their variances;
  4. the same expectation as rt_radiance_trace on three scenes, 2^20 paths each way;
  5. the side-pass manners of tests/test_gpu_radiance.py: the buffer form behind updates and held-back frames and into torch tensors,
     updates that turn emission on and off, no visible state change, every error row, the pass's own watchdog word;
  6. the entry cap through a context: RT_ERR_SCENE from the three calls, the scene still usable, and a table of exactly 2^22 entries;
  7. every device layout (RT_LAYOUT at rt_upload_scene): the visibility test names a triangle by hit_triangle(), which under `dense` divides
     the unit by 3 and under every other layout reads the unit -> triangle map, indexed in the triangle space or, under `arena`, in the
     pair space; a wrong index would only darken the picture.  Against the reference's records computed under the default layout;
  8. instances of one mesh with a real tree (scene nee_instances: two emissive models and a dark one share 320 triangles; the
     uploaded triangle index is the same for both, the object alone tells them apart);
  9. updates that move geometry: one context through a translation, a rotation with uneven scale, a mirroring transform, a moved and
     resized sphere, an identical update, the way back, an upload of another scene, a refused upload and the first scene again — the
     table holds world-space corners, areas, normals and probabilities, and a stale one gives plausible, wrong light.
The stack's last row under this kernel's two walks: tests/test_gpu_deep_trees.py."""
import ctypes as C
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deep_trees as dt  # noqa: E402
import nee_reference as nr  # noqa: E402
import radiance_reference as rr  # noqa: E402
import query_support as tq  # noqa: E402  (snapshot)
from flush_table import held_at  # noqa: E402
from gpu_support import DevBuf  # noqa: E402
from nee_support import (H, LAYOUTS, W, SceneArrays, assert_records, camera_batch, chained, grid_mesh, hip_tracer, scene,  # noqa: E402
                         without_cache)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
BIT_SCENES = ["nee_flat", "config3_bvh", "crowded70_emissive", "nee_mirrored", "nee_glass", "nee_inside", "nee_instances"]
BOUNCES = [-1, 0, 1, None]
LAYOUT_SCENES = ["config3_bvh", "crowded70_emissive", "nee_instances"]

_CASES = {}


def case(pkg, api, orc, name, bounce):
    """Scene, parameters, the 200 camera rays and the reference's records with what the batch covered: computed once, never written."""
    key = (name, bounce)
    if key not in _CASES:
        sc = scene(pkg, api, name)
        p, rays = camera_batch(pkg, api, orc, sc, W, H, bounce)
        tr = hip_tracer(api, sc, p)
        try:
            est = nr.Estimator(pkg, orc, tr, sc.models, sc.triangles, sc.spheres, p)
            want = est.trace(rays)
        finally:
            tr.close()
        for a in (rays, want):
            a.setflags(write=False)
        _CASES[key] = (sc, p, rays, want, est)
    return _CASES[key]


# ---------------------------------------------------------------- 1. bit for bit
@pytest.mark.parametrize("bounce", BOUNCES, ids=["bounce_-1", "bounce_0", "bounce_1", "bounce_default"])
@pytest.mark.parametrize("name", BIT_SCENES)
def test_records_equal_the_reference_bit_for_bit(pkg, api, orc, name, bounce):
    sc, p, rays, want, est = case(pkg, api, orc, name, bounce)
    assert np.isfinite(want["rgb"]).all(), "the reference's records of this case are not all finite"
    tr = hip_tracer(api, sc, p)
    try:
        got = tr.radiance_trace_nee(rays)
        prefixes = {k: tr.radiance_trace_nee(rays[:k]) for k in (1, 63, 64, 65)}
        plain = tr.radiance_trace(rays)
        counts = tr.nee_light_count()
    finally:
        tr.close()
    print(f"{name} bounce={p.maxBounceCount}: lights {counts}, {est.samples} samples ({est.triangle_samples} on triangles, {est.inside} inside their sphere), "
          f"{est.shadow_rays} shadow rays, {est.unshadowed} unshadowed, {est.suppressed} emissions left out")
    assert counts == (est.table["n_sphere_entries"], est.table["n_triangle_entries"]) and sum(counts) > 0
    assert_records(got, want, f"{name} bounce={p.maxBounceCount}")
    for k, part in prefixes.items():
        assert part.tobytes() == want[:k].tobytes(), f"n = {k}"
    if p.maxBounceCount < 0:
        assert not got["rgb"].any() and np.array_equal(got["rng"], rays["rng"])
        return
    # the case covers what it is there for
    assert est.samples > 0 and est.shadow_rays > 0 and est.unshadowed > 0
    assert got.tobytes() != plain.tobytes()
    if (p.maxBounceCount >= 1 and name in ("nee_flat", "config3_bvh")) or (bounce is None and name == "crowded70_emissive"):  # (where the emitters are large enough)
        assert est.suppressed > 0, "no bounce behind a sampled vertex found an emitter"
    if name in ("nee_flat", "crowded70_emissive"):
        assert est.triangle_samples > 0 and est.samples > est.triangle_samples, "both kinds of entry"
    if name in ("config3_bvh", "nee_mirrored"):
        assert est.triangle_samples == est.samples
    if name in ("nee_glass", "nee_mirrored"):
        assert est.shadow_rays > est.unshadowed, "some shadow ray must be blocked"
    if name == "nee_inside":
        assert est.inside > 0
    if name == "nee_instances" and bounce is None:
        instances_cover_what_they_are_there_for(pkg, sc, est)


def instances_cover_what_they_are_there_for(pkg, sc, est):
    """The mesh has a real tree, and the reference's shadow rays (its shadow_log) went to both emissive instances, to one uploaded
    triangle under both objects, and were blocked and let through towards each."""
    names = [m.name for m in sc.desc.models]
    first, second, dark = (len(sc.spheres) + names.index(k) for k in ("BallLight", "MirroredBallLight", "DarkBall"))
    mesh = sc.desc.models[names.index("BallLight")].Mesh
    count = mesh.triangle_count
    offsets = sc.models["triOffset"][[names.index(k) for k in ("BallLight", "MirroredBallLight", "DarkBall")]]
    assert count >= 200 and len(set(offsets.tolist())) == 1, "three models, one mesh"
    off, node_off = int(offsets[0]), int(sc.models["nodeOffset"][names.index("BallLight")])
    node_end = min([int(o) for o in sc.models["nodeOffset"] if o > node_off], default=len(sc.nodes))
    nodes = sc.nodes[node_off:node_end]
    assert (nodes["triangleCount"] <= 0).sum() > 8 and (nodes["triangleCount"] > 0).sum() > 8, "a tree with inner nodes and many leaf runs"
    given = mesh.vertices[mesh.triangles.reshape(-1, 3)[:, 0]]
    assert not np.array_equal(sc.triangles["posA"][off:off + count], given), "the builder reordered the triangles"
    assert np.linalg.det(sc.models["localToWorld"][names.index("MirroredBallLight")].reshape(4, 4)[:3, :3].astype(np.float64)) < 0
    log = est.shadow_log
    wanted = {obj: {t for (_, _, _, _, o, t, _) in log if o == obj} for obj in (first, second)}
    assert wanted[first] and wanted[second], "samples on both instances"
    assert all(off <= t < off + count for obj in wanted for t in wanted[obj])
    assert wanted[first] & wanted[second], "no uploaded triangle index was wanted under both objects"
    for obj in (first, second):
        seen = [s for (_, _, _, _, o, _, s) in log if o == obj]
        assert any(seen) and not all(seen), f"object {obj}: {sum(seen)} of {len(seen)} shadow rays unshadowed"
    assert not any(o == dark for (_, _, _, _, o, _, _) in log)
    assert est.suppressed > 0 and est.samples > est.triangle_samples > 0
    print(f"nee_instances: {len(wanted[first])} / {len(wanted[second])} triangles wanted on the two instances, {len(wanted[first] & wanted[second])} on both; "
          f"{est.suppressed} emissions left out")


def test_a_grid_of_two_waves_draws_its_blocks_from_the_counter(pkg, api, orc, monkeypatch):
    sc, p, rays, want, est = case(pkg, api, orc, "config3_bvh", None)
    monkeypatch.setenv("RT_GRID", "2")  # read at rt_create: four blocks, two waves
    tr = api.create_tracer(0)
    monkeypatch.delenv("RT_GRID")
    try:
        sc.upload(tr)
        tr.set_params(p)
        got = tr.radiance_trace_nee(rays)
        rev = tr.radiance_trace_nee(rays[::-1])[::-1]
    finally:
        tr.close()
    assert_records(got, want, "RT_GRID=2")
    assert rev.tobytes() == want.tobytes(), "reversed"


# ---------------------------------------------------------------- 2. the two identities
@pytest.mark.parametrize("name", BIT_SCENES)
def test_without_emitters_the_records_are_rt_radiance_traces(pkg, api, orc, name):
    sc = scene(pkg, api, name)
    models, spheres = sc.stripped()
    for bounce in (None, 1):
        p, rays = camera_batch(pkg, api, orc, sc, W, H, bounce)
        if name != "config3_bvh":
            p.useSky = 1  # (light from somewhere, so that the paths differ in more than their states)
        tr = hip_tracer(api, sc, p, models=models, spheres=spheres)
        try:
            assert tr.nee_light_count() == (0, 0)
            plain = tr.radiance_trace(rays)
            got = tr.radiance_trace_nee(rays)
        finally:
            tr.close()
        assert got.tobytes() == plain.tobytes(), f"{name} bounce={p.maxBounceCount}"
        assert (got["rng"] != rays["rng"]).any()


def test_an_all_mirror_scene_gives_rt_radiance_traces_records(pkg, api, orc):
    sc = scene(pkg, api, "nee_mirrors")
    p, rays = camera_batch(pkg, api, orc, sc, W, H, None)
    tr = hip_tracer(api, sc, p)
    try:
        assert tr.nee_light_count() == (1, 0)
        plain = tr.radiance_trace(rays)
        got = tr.radiance_trace_nee(rays)
    finally:
        tr.close()
    assert got.tobytes() == plain.tobytes()
    assert got["rgb"].any() and (got["rng"] != rays["rng"]).any()


# ---------------------------------------------------------------- 3. physics, closed form
@pytest.mark.parametrize("offset", [0.7, 2.0])
def test_floor_under_a_spherical_emitter_closed_form(pkg, api, orc, offset):
    """A diffuse floor (rho = 0.8) under an emissive sphere (r = 0.5, centre 3 above the floor, Le = 10, diffuseCol 0), no sky,
    maxBounceCount = 1, one ray straight down at the floor `offset` to the side: the reflected radiance is rho Le (r / d)^2 cos(theta_c),
    d and theta_c taken from the offset origin hit.pos + 0.001 n.  2^16 samples (256 chains of 256).  Both estimators within 5 standard
    errors (their own) + 2^-16 relative (fp32 over a few hundred operations); NEE's variance below 1/10 of the plain one's (expected:
    about 1e-4).  Then maxBounceCount = 0, 2^12 samples: plain radiance is 0 and NEE has the same closed form — the one bounce more of
    emitter light that the header states."""
    rho, le, r, height = 0.8, 10.0, 0.5, 3.0
    M, S = pkg.RayTracingMaterial, pkg.Sphere
    floor = pkg.Model(pkg.meshes.quad(), M(diffuseCol=(rho, rho, rho, 1), specularProbability=0.0), pkg.Transform((0, 0, 0), (90, 0, 0), (40, 40, 1)), "Floor")
    light = S((0, height, 0), r, M(diffuseCol=(0, 0, 0, 1), emissionCol=(1, 1, 1, 1), emissionStrength=le))
    cam = pkg.Camera(pkg.Transform((0, 1, -6)), fieldOfView=60.0)
    settings = dict(maxBounceCount=1, numRaysPerPixel=1, useSky=False, accumulate=True, bvhQuality=1)
    sc = SceneArrays(api, pkg.scenes.SceneDescription("nee_physics", 64, 36, 1, settings, cam, [floor], [light]))
    p = rr.params_of(sc, api, 64, 36, {})
    assert p.maxBounceCount == 1 and not p.useSky
    ray = pkg.abi.make_path_rays([[offset, 1.0, 0.0]], [[0, -1, 0]], 1)
    tr = hip_tracer(api, sc, p)
    try:
        hit = tr.query_closest(pkg.abi.make_rays(ray["origin"], ray["dir"]))[0]
        nee = chained(tr.radiance_trace_nee, ray, 256, 256)
        plain = chained(tr.radiance_trace, ray, 256, 256)
        p.maxBounceCount = 0  # the cut the header states: the sample at the last vertex carries one more bounce of emitter light
        tr.set_params(p)
        nee0 = chained(tr.radiance_trace_nee, ray, 256, 16)
        plain0 = chained(tr.radiance_trace, ray, 256, 16)
    finally:
        tr.close()
    assert hit["object"] == 1 and np.allclose(hit["normal"], (0, 1, 0), atol=1e-6)
    x = hit["pos"].astype(np.float64) + 0.001 * hit["normal"].astype(np.float64)
    to_c = np.array([0, height, 0]) - x
    d = np.linalg.norm(to_c)
    want = rho * le * (r / d) ** 2 * (to_c[1] / d)
    assert (nee[:, 0] == nee[:, 1]).all() and (nee[:, 0] == nee[:, 2]).all()
    n = len(nee)
    assert n == 1 << 16
    figures = {}
    for what, v in (("nee", nee[:, 0].astype(np.float64)), ("plain", plain[:, 0].astype(np.float64))):
        mean, var = v.mean(), v.var(ddof=1)
        se = np.sqrt(var / n)
        figures[what] = (mean, var, se)
        print(f"offset {offset}: {what}: mean {mean:.6f} (closed form {want:.6f}), standard error {se:.3e}, variance {var:.6e}")
    print(f"offset {offset}: variance ratio nee / plain = {figures['nee'][1] / figures['plain'][1]:.3e}")
    for what, (mean, var, se) in figures.items():
        assert abs(mean - want) <= 5 * se + 2.0 ** -16 * want, (what, mean, want, se)
    assert figures["nee"][1] < figures["plain"][1] / 10
    # maxBounceCount = 0: Trace sees the floor and nothing else; this pass returns the directly lit floor, the same closed form
    v0 = nee0[:, 0].astype(np.float64)
    se0 = np.sqrt(v0.var(ddof=1) / len(v0))
    print(f"offset {offset}: maxBounceCount 0: nee mean {v0.mean():.6f} (closed form {want:.6f}), standard error {se0:.3e}; plain: all zero")
    assert not plain0.any()
    assert abs(v0.mean() - want) <= 5 * se0 + 2.0 ** -16 * want, (v0.mean(), want, se0)


# ---------------------------------------------------------------- 4. the same expectation
@pytest.mark.parametrize("name", ["nee_flat", "config3_bvh", "nee_glass"])
def test_same_expectation_as_plain_radiance(pkg, api, orc, name):
    """2^20 paths each way over 24 x 16 camera rays (each ray 2,731 times with its own generator state), fixed seeds: per colour
    channel the two float64 means differ by at most 5 combined standard errors, each from its run's per-sample values."""
    sc = scene(pkg, api, name)
    p, cam = camera_batch(pkg, api, orc, sc, 24, 16, None)
    reps = -(-(1 << 20) // len(cam))
    rays = np.tile(cam, reps)
    rays["rng"] = (np.arange(len(rays), dtype=np.uint64) * 2654435761 + 977) % (1 << 32)
    assert len(rays) >= 1 << 20
    tr = hip_tracer(api, sc, p)
    try:
        nee = tr.radiance_trace_nee(rays)["rgb"].astype(np.float64)
        plain = tr.radiance_trace(rays)["rgb"].astype(np.float64)
    finally:
        tr.close()
    assert np.isfinite(nee).all() and np.isfinite(plain).all()
    n = len(rays)
    for c in range(3):
        m1, m2 = nee[:, c].mean(), plain[:, c].mean()
        s1, s2 = np.sqrt(nee[:, c].var(ddof=1) / n), np.sqrt(plain[:, c].var(ddof=1) / n)
        print(f"{name} channel {c}: nee {m1:.6f} +- {s1:.2e}, plain {m2:.6f} +- {s2:.2e}, difference {abs(m1 - m2) / np.hypot(s1, s2):.2f} combined standard errors, "
              f"variance ratio {nee[:, c].var() / plain[:, c].var():.3f}")
        assert m1 > 0 and m2 > 0
        assert abs(m1 - m2) <= 5 * np.hypot(s1, s2), (name, c, m1, m2, s1, s2)


# ---------------------------------------------------------------- 5. the side-pass manners
def test_buffer_form_sees_updates_and_runs_behind_held_back_frames(pkg, api, orc, forced=False):
    """A pass enqueued right behind rt_update_spheres sees the emitter it made (and the table rebuilt for it); passes between
    rt_render_frame calls that are held back leave the image what the same frames give without any pass."""
    abi = pkg.abi
    w, h = 64, 36
    images = []
    for with_passes in (True, False):
        tr = api.create_tracer(0)
        try:
            mgr = pkg.scenes.get(2).make_manager(tr, api, w, h)
            mgr.OnEnable(renderSeed=3)
            spheres = mgr._pack_spheres()
            n = 70
            rays = np.repeat(abi.make_path_rays([[0.0, 0.05, 0.0]], [[0, -1, 0]], 9), n)  # between the spheres, straight down at the ground
            rays["origin"][:, 0] += np.arange(n) * F(0.002)
            rays["rng"] = np.arange(n) + 100
            d_rays, d_out = DevBuf(rays.nbytes).upload(rays), DevBuf(n * 16)
            if with_passes:
                before = tr.radiance_trace_nee(rays)
                lights = tr.nee_light_count()
                assert lights == (2, 0)
            mgr.RenderFrames(5)
            for _ in range(3):  # rt_render_frame may hold these back
                mgr.RenderFrame()
                if with_passes:
                    held_at(tr, "test_gpu_nee: rt_nee_trace_buffers behind rt_render_frame", forced)
                    tr.radiance_trace_nee_buffers(d_rays.ptr, n, d_out.ptr)
            if with_passes:
                tr.synchronize()
                assert d_out.download(abi.RADIANCE_DTYPE).tobytes() == before.tobytes()
                changed = spheres.copy()
                changed["material"]["emissionStrength"][:] = 0  # every sphere put out ...
                changed["material"]["emissionCol"][0] = (0.5, 0.25, 0.125, 1)  # ... and one lit
                changed["material"]["emissionStrength"][0] = 2.0
                changed["material"]["flag"][0] = 0
                tr.update_spheres(changed)
                tr.radiance_trace_nee_buffers(d_rays.ptr, n, d_out.ptr)  # no synchronise in between
                tr.synchronize()
                seen = d_out.download(abi.RADIANCE_DTYPE)
                assert tr.nee_light_count() == (1, 0)
                fresh = api.create_tracer(0)
                try:
                    data = mgr.CreateAllMeshData(mgr.models)
                    fresh.upload_scene(data["meshInfo"], data["triangles"], data["nodes"], changed)
                    fresh.set_params(mgr.params())
                    assert seen.tobytes() == fresh.radiance_trace_nee(rays).tobytes(), "the pass behind the update != a context that was given the updated scene"
                finally:
                    fresh.close()
                assert seen.tobytes() != before.tobytes()
                assert seen.tobytes() == tr.radiance_trace_nee(rays).tobytes(), "buffer form vs host form"
                tr.update_spheres(spheres)  # back, for the frames that follow
                assert tr.nee_light_count() == (2, 0)
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


def test_updates_that_turn_a_models_emission_on_and_off_are_seen(pkg, api, orc):
    sc, p, rays, want, est = case(pkg, api, orc, "config3_bvh", None)
    names = [m.name for m in sc.desc.models]
    light, cube = names.index("Light"), names.index("OpaqueRoundedCube")
    tri_count = [m.Mesh.triangle_count for m in sc.desc.models]
    tr = hip_tracer(api, sc, p)
    try:
        assert tr.nee_light_count() == (0, tri_count[light])
        assert tr.radiance_trace_nee(rays).tobytes() == want.tobytes()
        off = sc.models.copy()
        off["material"]["emissionStrength"][light] = 0
        tr.update_models(off)
        assert tr.nee_light_count() == (0, 0)
        dark = tr.radiance_trace_nee(rays)
        assert dark.tobytes() == tr.radiance_trace(rays).tobytes() and not dark["rgb"].any()
        on = off.copy()
        on["material"]["emissionCol"][cube] = (1, 0.5, 0.2, 1)
        on["material"]["emissionStrength"][cube] = 4.0
        tr.update_models(on)
        lit = tr.radiance_trace_nee(rays)  # the pass itself rebuilds the table
        assert tr.nee_light_count() == (0, tri_count[cube])
        fresh = hip_tracer(api, sc, p, models=on)
        try:
            assert lit.tobytes() == fresh.radiance_trace_nee(rays).tobytes()
        finally:
            fresh.close()
        assert lit["rgb"].any()
        tr.update_models(sc.models)
        assert tr.nee_light_count() == (0, tri_count[light])
        assert tr.radiance_trace_nee(rays).tobytes() == want.tobytes()
    finally:
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
abi = pkg.abi
rng = np.random.default_rng(5)
for cfg in (3, 2):
    tr = api.create_tracer(0)
    mgr = pkg.scenes.get(cfg).make_manager(tr, api, 64, 36)
    mgr.InitBVH()  # the scene ...
    mgr.SetShaderParams()  # ... and the parameters, no image
    n = 1000
    o = rng.normal(size=(n, 3)); o = 2.5 * o / np.linalg.norm(o, axis=1, keepdims=True) + [0, 2, 0]
    d = rng.uniform(-2, 2, (n, 3)) + [0, 1, 0] - o
    rays = abi.make_path_rays(o, d, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))
    host = tr.radiance_trace_nee(rays)
    assert host["rgb"].any() and (host["rng"] != rays["rng"]).any()
    assert host.tobytes() != tr.radiance_trace(rays).tobytes()
    t_rays = torch.from_numpy(rays.view(np.uint32).reshape(n, 8).copy().view(np.int32)).to("cuda:0")
    t_out = torch.full((n, 4), 0x7fc00001, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    tr.radiance_trace_nee_buffers(t_rays.data_ptr(), n, t_out.data_ptr())
    tr.synchronize()
    assert t_out.cpu().numpy().tobytes() == host.tobytes(), "tensor != host form (config %d)" % cfg
    # on the caller's stream (rt_set_stream): work enqueued on that stream behind the pass sees its records
    s = torch.cuda.Stream()
    tr.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        t2 = torch.zeros((n, 4), dtype=torch.int32, device="cuda:0")
        s.synchronize()
        tr.radiance_trace_nee_buffers(t_rays.data_ptr(), n, t2.data_ptr())
        copy = t2.clone()
    s.synchronize()
    assert copy.cpu().numpy().tobytes() == host.tobytes(), "stream order (config %d)" % cfg
    tr.set_stream(None)
    tr.synchronize()
    tr.close()
print("NEE_TORCH_OK")
"""


def test_buffer_form_into_torch_tensors(pkg, api):
    """rt_nee_trace_buffers on torch tensors' data_ptr()s == the host form, and in the order of a torch stream given to
    rt_set_stream.  In a child process that imports torch first, so that the library shares torch's HIP runtime."""
    p = subprocess.run([sys.executable, "-c", _TORCH_CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "NEE_TORCH_OK" in p.stdout, "rc=%d\n%s\n%s" % (p.returncode, p.stdout[-3000:], p.stderr[-3000:])


def mixed_calls(tr, rays, bufs):
    d_rays, d_out = bufs
    n = len(rays)
    out = tr.radiance_trace_nee(rays)
    tr.radiance_trace_nee_buffers(d_rays.ptr, n, d_out.ptr)
    tr.synchronize()
    assert d_out.download(np.uint8).tobytes() == out.tobytes()
    assert tr.radiance_trace_nee(rays[:0]).shape == (0,)
    assert tr.nee_light_count()[1] > 0
    return out


def test_nee_calls_leave_no_trace(pkg, api, orc):
    sc, p, rays, want, est = case(pkg, api, orc, "config3_bvh", None)
    n = len(rays)
    bufs = (DevBuf(n * 32).upload(rays), DevBuf(n * 16))
    try:
        # a rendering context, whole and as part 1 of 2 of a strip partition: everything a caller can read is the same before and after,
        # and so are the records of the other passes (whose watchdog words a synchronise would report)
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
            others = (tr.radiance_trace(rays).tobytes(), tr.query_closest(pkg.abi.make_rays(rays["origin"], rays["dir"])).tobytes())
            before = tq.snapshot(tr)
            assert before["counters"]["segments"] > 0
            got = mixed_calls(tr, rays, bufs)
            tr.synchronize()
            after = tq.snapshot(tr)
            assert before == after, [k for k in before if before[k] != after[k]]
            assert others == (tr.radiance_trace(rays).tobytes(), tr.query_closest(pkg.abi.make_rays(rays["origin"], rays["dir"])).tobytes())
            assert got["rgb"].any()
            tr.close()
    finally:
        for b in bufs:
            b.free()


def test_errors(pkg, api, orc):
    abi = pkg.abi
    sc, p, rays200, want, est = case(pkg, api, orc, "config3_bvh", None)
    n = 100
    rays = rays200[:n].copy()
    out = np.zeros(n, dtype=abi.RADIANCE_DTYPE)
    d_rays, d_out = DevBuf(n * 32).upload(rays), DevBuf(n * 16)
    bad, state, ok = abi.RT_ERR_INVALID_ARG, abi.RT_ERR_STATE, abi.RT_OK
    host, dev = api.nee_trace, api.nee_trace_buffers
    a, b = C.c_int(-7), C.c_int(-7)
    tr = api.create_tracer(0)
    try:
        tr.set_params(p)  # parameters, no scene
        assert host(tr.h, rays.ctypes.data, n, out.ctypes.data) == state and b"rt_upload_scene" in api.last_error(tr.h)
        assert dev(tr.h, d_rays.ptr, n, d_out.ptr) == state and b"rt_upload_scene" in api.last_error(tr.h)
        assert api.nee_light_count(tr.h, C.byref(a), C.byref(b)) == state and b"rt_upload_scene" in api.last_error(tr.h) and (a.value, b.value) == (-7, -7)
        tr.close()
        tr = sc.upload(api.create_tracer(0))  # a scene, no parameters
        assert host(tr.h, rays.ctypes.data, n, out.ctypes.data) == state and b"rt_set_params" in api.last_error(tr.h)
        assert dev(tr.h, d_rays.ptr, n, d_out.ptr) == state and b"rt_set_params" in api.last_error(tr.h)
        assert api.nee_light_count(tr.h, C.byref(a), C.byref(b)) == ok and (a.value, b.value) == (0, 12)  # (the table needs no parameters)
        assert api.nee_light_count(tr.h, None, None) == ok
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
        assert out.tobytes() == want[:n].tobytes(), "after the errors"
        assert d_out.download(np.uint8).tobytes() == out.tobytes()
    finally:
        tr.close()
        d_rays.free(), d_out.free()


def test_watchdog_fails_the_pass_not_the_context(pkg, api, orc, monkeypatch):
    """RT_TRAV_LIMIT=4 (read at rt_upload_scene; the step limit is a software counter, nothing can hang): the walks of the pass are cut
    short.  The host form says so when it returns, the buffer form at the next rt_synchronize or rt_nee_trace* call, once;
    the frames the context rendered before stay readable; the plain radiance pass reports its own word only."""
    abi = pkg.abi
    sc, p, rays, want, est = case(pkg, api, orc, "config3_bvh", None)
    n = len(rays)
    bufs = (DevBuf(n * 32).upload(rays), DevBuf(n * 16))
    tr = api.create_tracer(0)
    try:
        mgr = pkg.scenes.get(3).make_manager(tr, api, 24, 16)
        mgr.OnEnable(renderSeed=1)
        mgr.RenderFrames(2)
        image = tr.read_accumulated().tobytes()
        monkeypatch.setenv("RT_TRAV_LIMIT", "4")
        sc.upload(tr)  # the limit of a scene is set when it is uploaded; the images stay
        monkeypatch.delenv("RT_TRAV_LIMIT")

        def reported(e, call, *holds):
            msg = str(e.value)
            assert e.value.status == abi.RT_ERR_HIP and "watchdog" in msg, msg
            assert msg.startswith(f"rt status {abi.RT_ERR_HIP}: {call}: "), msg
            for text in holds:
                assert text in msg, (text, msg)
            return msg
        family = "in the pass of an rt_nee_trace_buffers call"
        with pytest.raises(abi.RtError) as e:
            tr.radiance_trace_nee(rays)
        reported(e, "rt_nee_trace", "in this pass", "the records are not valid")
        tr.radiance_trace_nee_buffers(bufs[0].ptr, n, bufs[1].ptr)  # enqueued: RT_OK
        with pytest.raises(abi.RtError) as e:
            tr.synchronize()
        reported(e, "rt_synchronize", family)
        tr.synchronize()  # reported once
        tr.radiance_trace_nee_buffers(bufs[0].ptr, n, bufs[1].ptr)
        with pytest.raises(abi.RtError) as e:  # the next call of the family reports it if it comes first ...
            tr.radiance_trace_nee_buffers(bufs[0].ptr, n, bufs[1].ptr)
        reported(e, "rt_nee_trace_buffers", family)
        tr.synchronize()  # ... once (and the call that reported enqueued nothing)
        # the plain radiance pass neither reports it nor is failed by it: it says what its own pass met
        tr.radiance_trace_nee_buffers(bufs[0].ptr, n, bufs[1].ptr)
        with pytest.raises(abi.RtError) as e:
            tr.radiance_trace(rays)
        assert "nee" not in reported(e, "rt_radiance_trace", "in this pass")
        with pytest.raises(abi.RtError) as e:
            tr.synchronize()
        reported(e, "rt_synchronize", family)
        tr.synchronize()
        assert tr.frame() == 3
        assert tr.read_accumulated().tobytes() == image  # RT_OK: the context's watchdog word was not set
        sc.upload(tr)
        tr.set_params(p)
        assert tr.radiance_trace_nee(rays).tobytes() == want.tobytes(), "after the re-upload"
    finally:
        tr.close()
        for b in bufs:
            b.free()


# ---------------------------------------------------------------- 6. the entry cap, through a context
def test_more_entries_than_the_cap_is_a_scene_error_of_these_calls_only(pkg, api, orc):
    """One mesh of 2^16 triangles under 65 emissive models: 65 x 2^16 entries, 2^16 past RT_NEE_MAX_LIGHTS, from 2^16 uploaded
    triangles.  The three calls of the header refuse with RT_ERR_SCENE and say why, every time (the table stays stale); the scene stays
    usable by every other call; and once an update puts one model out the table has exactly 2^22 entries and the pass runs — the
    bounded search at its largest table."""
    abi = pkg.abi
    M, T = pkg.RayTracingMaterial, pkg.Transform
    mesh = grid_mesh(pkg)
    assert mesh.triangle_count == 1 << 16
    lit = dict(diffuseCol=(0, 0, 0, 1), emissionCol=(1, 0.9, 0.8, 1), emissionStrength=3.0)
    models = [pkg.Model(mesh, M(**lit), T((0, 0.05 * k, 3 + 0.02 * k), (0, 0, 0), (2.0, 1.0, 1)), f"Panel{k}") for k in range(65)]
    models.append(nr._floor(pkg))  # a diffuse floor in front of the panels: its vertices sample them
    cam = pkg.Camera(T((0, 1, -4)), fieldOfView=60.0)
    settings = dict(maxBounceCount=2, numRaysPerPixel=1, useSky=False, accumulate=True, bvhQuality=1)
    sc = SceneArrays(api, pkg.scenes.SceneDescription("nee_cap", 64, 36, 1, settings, cam, models, []))
    assert len(sc.triangles) == (1 << 16) + 2 and len(set(sc.models["triOffset"][:65])) == 1
    p, rays = camera_batch(pkg, api, orc, sc, 16, 8, None)
    n = len(rays)
    out = np.zeros(n, dtype=abi.RADIANCE_DTYPE)
    d_rays, d_out = DevBuf(n * 32).upload(rays), DevBuf(n * 16)
    a, b = C.c_int(-7), C.c_int(-7)
    tr = hip_tracer(api, sc, p)
    try:
        for _ in range(2):
            assert api.nee_trace(tr.h, rays.ctypes.data, n, out.ctypes.data) == abi.RT_ERR_SCENE
            assert api.last_error(tr.h).startswith(b"rt_nee_trace: ") and b"RT_NEE_MAX_LIGHTS" in api.last_error(tr.h)
            assert api.nee_trace_buffers(tr.h, d_rays.ptr, n, d_out.ptr) == abi.RT_ERR_SCENE
            assert api.last_error(tr.h).startswith(b"rt_nee_trace_buffers: ") and b"RT_NEE_MAX_LIGHTS" in api.last_error(tr.h)
            assert api.nee_light_count(tr.h, C.byref(a), C.byref(b)) == abi.RT_ERR_SCENE and (a.value, b.value) == (-7, -7)
            assert api.last_error(tr.h).startswith(b"rt_nee_light_count: ") and b"RT_NEE_MAX_LIGHTS" in api.last_error(tr.h)
        tr.synchronize()  # nothing was enqueued, nothing is pending
        assert not out.view(np.uint32).any() and not d_out.download(np.uint32).any(), "a refused call wrote records"
        plain = tr.radiance_trace(rays)  # the scene itself stays usable
        hits = tr.query_closest(abi.make_rays(rays["origin"], rays["dir"]))
        assert plain["rgb"].any() and (hits["object"] >= 0).any()
        fewer = sc.models.copy()
        fewer["material"]["emissionStrength"][64] = 0  # one panel put out: 64 x 2^16 = the cap exactly
        tr.update_models(fewer)
        assert tr.nee_light_count() == (0, abi.NEE_MAX_LIGHTS)
        got = tr.radiance_trace_nee(rays)
        tr.radiance_trace_nee_buffers(d_rays.ptr, n, d_out.ptr)
        tr.synchronize()
        assert d_out.download(abi.RADIANCE_DTYPE).tobytes() == got.tobytes()
        assert np.isfinite(got["rgb"]).all() and got["rgb"].any() and got.tobytes() != tr.radiance_trace(rays).tobytes()
        tr.update_models(sc.models)  # and back past the cap
        assert api.nee_light_count(tr.h, C.byref(a), C.byref(b)) == abi.RT_ERR_SCENE
        assert tr.radiance_trace(rays).tobytes() == plain.tobytes()
    finally:
        tr.close()
        d_rays.free(), d_out.free()


# ---------------------------------------------------------------- 7. every device layout
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", LAYOUT_SCENES)
def test_every_device_layout_gives_the_references_records(pkg, api, orc, monkeypatch, capfd, name, layout):
    """RT_LAYOUT is read by rt_upload_scene (prepare_scene), not by rt_create: it stays set until the scene is uploaded, and the upload's
    own report (RT_DEBUG_UPLOAD) must name the layout asked for — a context that took the default, or a scene that silently fell back
    to `dense`, would make the case empty."""
    t0 = time.perf_counter()
    monkeypatch.delenv("RT_LAYOUT", raising=False)
    sc, p, rays, want, est = case(pkg, api, orc, name, None)  # the reference walked its rays under the default layout
    used = api.layout_arrays(sc.models, sc.triangles, sc.nodes, layout)["used"]  # (no device needed)
    assert without_cache(used) == without_cache(layout), f"asked for {layout}, the scene is laid out as {used}"
    assert (used == "dense") == (layout == "dense")
    monkeypatch.setenv("RT_LAYOUT", layout)
    monkeypatch.setenv("RT_DEBUG_UPLOAD", "1")
    tr = api.create_tracer(0)
    try:
        capfd.readouterr()
        sc.upload(tr)
        reported = re.findall(r"prepare_scene: layout (\S+)", capfd.readouterr().err)
        monkeypatch.delenv("RT_LAYOUT")
        monkeypatch.delenv("RT_DEBUG_UPLOAD")
        tr.set_params(p)
        got = tr.radiance_trace_nee(rays)
        counts = tr.nee_light_count()
    finally:
        tr.close()
    assert [without_cache(r) for r in reported] == [without_cache(used)], f"asked for {layout}: the upload reports {reported}, rt_debug_layout {used}"
    assert_records(got, want, f"{name}, RT_LAYOUT={layout}")
    assert got.tobytes() == want.tobytes()
    assert counts == (est.table["n_sphere_entries"], est.table["n_triangle_entries"])
    assert est.triangle_samples > 0, "no vertex sampled a triangle entry"
    on_triangles = [seen for (_, _, _, _, _, tri, seen) in est.shadow_log if tri >= 0]
    assert any(on_triangles) and est.unshadowed > 0, "no shadow ray towards a triangle entry was unshadowed: a wrong triangle index would not show"
    print(f"{name}, RT_LAYOUT={layout} (used: {used}): {sum(on_triangles)} of {len(on_triangles)} shadow rays towards triangles unshadowed; {time.perf_counter() - t0:.1f} s")


# ---------------------------------------------------------------- 9. updates that move geometry
def with_transform(pkg, models, index, matrix):
    """A copy of the model array with model `index` under the 4 x 4 localToWorld `matrix`"""
    out = models.copy()
    m = np.asarray(matrix, dtype=np.float64)
    out["localToWorld"][index] = pkg.manager.matrix_to_abi(m)
    out["worldToLocal"][index] = pkg.manager.matrix_to_abi(np.linalg.inv(m))
    return out


def test_one_context_through_updates_that_move_emitters(pkg, api, orc):
    """The steps of the module text's item 9.  After every step: a buffer-form call enqueued right behind it (no synchronise), then the
    host form; both == a fresh context that was given the step's arrays; rt_nee_light_count == that context's == the numpy table's; on
    the steps marked so, also == the reference rebuilt from the step's arrays."""
    abi = pkg.abi
    t0 = time.perf_counter()
    first, other = scene(pkg, api, "nee_flat"), scene(pkg, api, "nee_instances")
    p, rays = camera_batch(pkg, api, orc, first, 16, 8, 2)
    n = len(rays)
    names = [m.name for m in first.desc.models]
    light = names.index("QuadLight")
    T = pkg.Transform
    assert nr.light_table(abi, first.models, first.triangles, first.spheres)["in_table"][len(first.spheres) + light]
    moved = with_transform(pkg, first.models, light, T((-0.7, 3.0, 0.6), (-90, 0, 0), (1.5, 1.0, 1)).localToWorldMatrix)
    turned = with_transform(pkg, first.models, light, T((-0.7, 3.0, 0.6), (-70, 25, 10), (2.2, 0.6, 1)).localToWorldMatrix)
    mirror = np.array([[1.5, 0, 0, 0.3], [0, 0, 1, 2.5], [0, 1.2, 0, 0.2], [0, 0, 0, 1]], dtype=np.float64)  # (nee_mirrored's: local -z -> world -y)
    assert np.linalg.det(mirror[:3, :3]) < 0
    mirrored = with_transform(pkg, first.models, light, mirror)
    spheres = first.spheres.copy()
    assert spheres["material"]["emissionStrength"][1] > 0
    spheres["centre"][1], spheres["radius"][1] = (-1.5, 2.8, -0.3), 2 * first.spheres["radius"][1]
    deep = dt.one_model(pkg, *dt.comb(abi, 33))  # 33 levels: refused

    d_rays, d_out = DevBuf(n * 32).upload(rays), DevBuf(n * 16)
    tr = api.create_tracer(0)
    records, lines = {}, []

    def check(step, arrays, reference):
        """Called right behind the step's update or upload."""
        tr.radiance_trace_nee_buffers(d_rays.ptr, n, d_out.ptr)  # no synchronise in between
        host = tr.radiance_trace_nee(rays)
        tr.synchronize()
        behind = d_out.download(abi.RADIANCE_DTYPE)
        counts = tr.nee_light_count()
        models, triangles, nodes, sph = arrays
        table = nr.light_table(abi, models, triangles, sph)
        fresh = api.create_tracer(0)
        try:
            fresh.upload_scene(models, triangles, nodes, sph)
            fresh.set_params(p)
            want = fresh.radiance_trace_nee(rays)
            assert fresh.nee_light_count() == counts, step
            if reference:
                est = nr.Estimator(pkg, orc, fresh, models, triangles, sph, p)
                ref = est.trace(rays)
                assert_records(host, ref, f"step {step} against the reference")
                assert est.shadow_rays > est.unshadowed > 0, step
        finally:
            fresh.close()
        assert counts == (table["n_sphere_entries"], table["n_triangle_entries"]) and sum(counts) > 0, (step, counts)
        assert behind.tobytes() == want.tobytes(), f"step {step}: the pass enqueued behind it != a context that was given its arrays"
        assert host.tobytes() == want.tobytes(), f"step {step}: host form"
        assert np.isfinite(host["rgb"]).all() and host["rgb"].any()
        records[step] = (host, counts)
        lines.append(f"step {step}: lights {counts}")
        return host

    try:
        tr.upload_scene(first.models, first.triangles, first.nodes, first.spheres)
        tr.set_params(p)
        at_first = (first.models, first.triangles, first.nodes, first.spheres)
        check("0", at_first, False)
        tr.update_models(moved)
        check("a", (moved, first.triangles, first.nodes, first.spheres), True)
        tr.update_models(turned)
        check("b", (turned, first.triangles, first.nodes, first.spheres), False)
        tr.update_models(mirrored)
        check("c", (mirrored, first.triangles, first.nodes, first.spheres), True)
        for prev, step in (("0", "a"), ("a", "b"), ("b", "c")):  # otherwise the update was not seen
            assert records[step][0].tobytes() != records[prev][0].tobytes(), f"step {step} left the records of step {prev}"
        tr.update_spheres(spheres)
        check("d", (mirrored, first.triangles, first.nodes, spheres), True)
        assert records["d"][0].tobytes() != records["c"][0].tobytes()
        tr.update_models(mirrored.copy())  # byte-identical updates
        tr.update_spheres(spheres.copy())
        check("e", (mirrored, first.triangles, first.nodes, spheres), False)
        assert records["e"][0].tobytes() == records["d"][0].tobytes() and records["e"][1] == records["d"][1]
        tr.update_models(first.models)
        tr.update_spheres(first.spheres)
        check("f", at_first, False)
        assert records["f"][0].tobytes() == records["0"][0].tobytes() and records["f"][1] == records["0"][1]
        assert (len(other.triangles), len(other.models), len(other.spheres)) != (len(first.triangles), len(first.models), len(first.spheres))
        tr.upload_scene(other.models, other.triangles, other.nodes, other.spheres)
        at_other = (other.models, other.triangles, other.nodes, other.spheres)
        check("g", at_other, True)
        assert records["g"][1] != records["0"][1]
        with pytest.raises(abi.RtError) as e:
            tr.upload_scene(*deep, None)
        assert e.value.status == abi.RT_ERR_SCENE and "BVH depth 33 > 32" in str(e.value), str(e.value)
        check("h", at_other, False)
        assert records["h"][0].tobytes() == records["g"][0].tobytes() and records["h"][1] == records["g"][1]
        tr.upload_scene(first.models, first.triangles, first.nodes, first.spheres)
        check("i", at_first, False)
        assert records["i"][0].tobytes() == records["0"][0].tobytes() and records["i"][1] == records["0"][1]
    finally:
        tr.close()
        d_rays.free(), d_out.free()
    print("\n".join(lines + [f"{time.perf_counter() - t0:.1f} s"]))
