"""rt_mis_trace (include/rt_mis.h) on the GPU.

  1. bit for bit, rgb and rng, against tests/mis_reference.py (the header's estimator restated path by path over rt_query_closest, the
     oracle's draws and functions, and a numpy light table and reverse map): the 200 camera rays of tests/test_gpu_nee.py,
     maxBounceCount -1, 0, 1, 2 and the scene's own, on its seven scenes; what each case covered is asserted from the reference's logs;
  2. block boundaries: n = 1, 63, 64, 65, 129, and 200 rays with the grid held to two waves;
  3. the identities: no emitters, an all-mirror scene and maxBounceCount = 0 give rt_radiance_trace's bits, on a BVH and a flat scene;
  4. physics in closed form: the floor under a spherical emitter, and a ceiling point 4 cm from a quad light against Lambert's
     polygon form factor;
  5. the bound of the header, record by record, where rt_nee_trace exceeds it;
  6. the same expectation as rt_radiance_trace at maxBounceCount 1 and the scene's own, 2^20 paths;
  7. the side-pass manners: behind held-back frames (the call's two `flushes` rows of tests/flush_table.py, once more with the records compared), behind updates,
     mixed with the other estimators, every error row, the cap, the pass's own watchdog word, torch tensors, every device layout;
  8. a lane that takes a second ray: one wave, a path that dies with its cosine set, then a ray whose first hit is an emitter;
  9. the rules of emission_weight: RULE_TABLE names the case that reaches each, or why no table the library builds can; no reference
     run of any MIS test may log one that is marked unreachable (rules_allowed).
The stack's last row, more than 64 models and non-finite values under this kernel: tests/test_gpu_deep_trees.py (g),
tests/test_gpu_many_models.py (e), tests/test_gpu_hazards.py."""
import ctypes as C
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mis_reference as mr  # noqa: E402
import nee_reference as nr  # noqa: E402
import nee_support as gn  # noqa: E402  (scenes, batches, helpers: shared, never written)
import query_support as tq  # noqa: E402
import radiance_reference as rr  # noqa: E402
from flush_table import held_at  # noqa: E402
from gpu_support import DevBuf  # noqa: E402
from mis_reference import RULE_TABLE, rules_allowed  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
W, H = gn.W, gn.H  # the 200 camera rays of tests/test_gpu_nee.py's bit test
BIT_SCENES = ["nee_flat", "config3_bvh", "crowded70_emissive", "nee_mirrored", "nee_glass", "nee_inside", "nee_instances"]
BOUNCES = [-1, 0, 1, 2, None]
_CASES = {}


def case(pkg, api, orc, name, bounce):
    """Scene, parameters, the 200 camera rays and the reference's records with its logs: computed once, never written."""
    key = (name, bounce)
    if key not in _CASES:
        sc = gn.scene(pkg, api, name)
        p, rays = gn.camera_batch(pkg, api, orc, sc, W, H, bounce)
        tr = gn.hip_tracer(api, sc, p)
        try:
            est = mr.Estimator(pkg, orc, tr, sc.models, sc.triangles, sc.spheres, p)
            want = est.trace(rays)
        finally:
            tr.close()
        for a in (rays, want):
            a.setflags(write=False)
        _CASES[key] = (sc, p, rays, want, est)
    return _CASES[key]


def weighted(est, kind):
    return [e for e in est.emission_log if e[3] == mr.WEIGHTED and 0.0 < e[2] < 1.0 and e[4] == kind]


# ---------------------------------------------------------------- 1. bit for bit
@pytest.mark.parametrize("bounce", BOUNCES, ids=["bounce_-1", "bounce_0", "bounce_1", "bounce_2", "bounce_default"])
@pytest.mark.parametrize("name", BIT_SCENES)
def test_records_equal_the_reference_bit_for_bit(pkg, api, orc, name, bounce):
    sc, p, rays, want, est = case(pkg, api, orc, name, bounce)
    assert np.isfinite(want["rgb"]).all(), "the reference's records of this case are not all finite"
    tr = gn.hip_tracer(api, sc, p)
    try:
        got = tr.radiance_trace_mis(rays)
        plain = tr.radiance_trace(rays)
    finally:
        tr.close()
    seen = sum(1 for s in est.sample_log if s[4])
    print(f"{name} bounce={p.maxBounceCount}: {est.samples} samples ({est.triangle_samples} on triangles), {len(est.sample_log)} shadow rays, {seen} added; "
          f"{len(est.emission_log)} emissions behind a sample: " + ", ".join(f"{r}: {sum(1 for e in est.emission_log if e[3] == r)}" for r in sorted({e[3] for e in est.emission_log})) +
          f"; {len(est.skipped_log)} last-vertex samples skipped, {len(est.plain_emission_log)} emitter hits behind no sample")
    gn.assert_records(got, want, f"{name} bounce={p.maxBounceCount}")
    assert got.tobytes() == want.tobytes()
    rules_allowed(est, f"{name} bounce={p.maxBounceCount}")
    for (_, _, g, _, _) in est.sample_log:
        assert 0.0 <= g <= 1.0
    for (_, _, wb, _, _) in est.emission_log:
        assert 0.0 <= wb <= 1.0
    if p.maxBounceCount < 0:
        assert not got["rgb"].any() and np.array_equal(got["rng"], rays["rng"])
        return
    if p.maxBounceCount == 0:  # an identity of the header: nothing is drawn, nothing is sampled
        assert est.samples == 0 and not est.emission_log and got.tobytes() == plain.tobytes()
        assert len(est.skipped_log) > 0
        return
    # the case covers what it is there for
    assert est.samples > 0 and len(est.sample_log) > 0
    assert got.tobytes() != plain.tobytes()
    assert all(v < p.maxBounceCount for (_, v, *_r) in est.sample_log) and all(v == p.maxBounceCount for (_, v) in est.skipped_log)
    if p.maxBounceCount == 2:  # the smallest count at which vertex 0 and vertex 1 sample and vertex 2 must not
        if name != "nee_mirrored":  # (its only emitter faces the floor: a path that reaches vertex 2 there is rare in 200 rays)
            assert {v for (_, v, *_r) in est.sample_log} == {0, 1}
    if bounce is None:
        assert seen > 0, "no sample of the default-bounce case was added"
        if name in ("nee_flat", "nee_instances"):
            assert weighted(est, "sphere"), "no emission with 0 < wb < 1 on a sphere"
            assert weighted(est, "triangle"), "no emission with 0 < wb < 1 on a triangle"
        if name == "nee_inside":
            assert any(e[3] == mr.INSIDE for e in est.emission_log), "no sphere hit from inside behind a sampled vertex"


def test_a_skipped_last_vertex_ends_the_path_and_emission_behind_no_sample_is_unweighted(pkg, api, orc):
    """At the last vertex nothing is drawn: the path ends there (Trace's loop runs out), so no emission can follow it.  What follows a
    vertex WITHOUT a sample — the first hit, or a hit behind a specular vertex — is added in full; nee_flat has both a skipped last
    vertex and such an emitter hit in one batch."""
    sc, p, rays, want, est = case(pkg, api, orc, "nee_flat", 1)
    assert est.skipped_log and est.plain_emission_log
    ended = {(i, v) for (i, v) in est.skipped_log}
    assert not any((i, v - 1) in ended for (i, v, *_r) in est.emission_log), "an emission was weighted behind a vertex that took no sample"
    assert not any((i, v - 1) in ended for (i, v, *_r) in est.segment_log), "a path went on behind its last vertex"


# ---------------------------------------------------------------- 2. block boundaries
def test_block_boundaries_and_a_grid_of_two_waves(pkg, api, orc, monkeypatch):
    sc, p, rays, want, est = case(pkg, api, orc, "config3_bvh", None)
    tr = gn.hip_tracer(api, sc, p)
    try:
        for k in (1, 63, 64, 65, 129):
            part = tr.radiance_trace_mis(rays[:k])
            assert part.tobytes() == want[:k].tobytes(), f"n = {k}"
    finally:
        tr.close()
    monkeypatch.setenv("RT_GRID", "2")  # read at rt_create: four blocks, two waves
    tr = api.create_tracer(0)
    monkeypatch.delenv("RT_GRID")
    try:
        sc.upload(tr)
        tr.set_params(p)
        got = tr.radiance_trace_mis(rays)
        rev = tr.radiance_trace_mis(rays[::-1])[::-1]
    finally:
        tr.close()
    gn.assert_records(got, want, "RT_GRID=2")
    assert rev.tobytes() == want.tobytes(), "reversed"


def test_a_reused_lane_starts_without_the_dead_paths_cosine(pkg, api, orc, monkeypatch):
    """One wave (RT_GRID=1, read at rt_create) and 128 rays: every lane takes a second ray when its first path has ended, and the feed's
    RT_FEED_START resets the lane's cnPrev (rt_nee_trace: prevSampled).  Half A, 64 of the 200 camera rays of nee_flat at
    maxBounceCount 1 whose path samples at vertex 0 and goes on into a segment that leaves the scene: no further vertex is shaded (one
    would set cnPrev to 0 itself: vertex 1 takes no sample), so the lane's path ends with cnPrev = cn' > 0.  Half B, 64 rays aimed
    straight at the emissive sphere, which has an entry: the first hit is an emitter, added in full — weighted by a dead path's cosine it
    would be wb < 1 of it.  A then B, and B then A: the reference's records, and B's the same bytes in both orders."""
    t0 = time.perf_counter()
    abi = pkg.abi
    sc, p, cam, _, est = case(pkg, api, orc, "nee_flat", 1)
    assert p.maxBounceCount == 1
    sampled = {i for (i, v, *_r) in est.sample_log if v == 0}
    went_on = {i for (i, v, _, _) in est.segment_log if v == 1}
    shaded_again = {i for (i, v, *_r) in est.emission_log if v == 1}   # (no glass in nee_flat: every hit of a second segment is an opaque one, and logged here)
    assert not (sc.models["material"]["flag"] == abi.MATERIAL_GLASS).any() and not (sc.spheres["material"]["flag"] == abi.MATERIAL_GLASS).any()
    keep = sorted((sampled & went_on) - shaded_again)
    assert len(keep) >= 16, f"only {len(keep)} of the 200 camera rays sample at vertex 0 and then leave the scene"
    half_a = cam[np.resize(np.array(keep), 64)]
    emitter = 1   # sphere 1: r = 0.4 at (-2.5, 2.5, 0.5), Le = 9, diffuseCol 0
    centre, radius = sc.spheres["centre"][emitter].astype(np.float64), float(sc.spheres["radius"][emitter])
    assert est.table["in_table"][emitter] and radius == F(0.4)
    k = np.arange(64)
    phi, cos_t = 2.399963 * k, 0.15 + 0.8 * (k + 0.5) / 64     # a spiral over the upper half of directions: nothing stands between
    u = np.stack([np.sqrt(1 - cos_t ** 2) * np.cos(phi), cos_t, np.sqrt(1 - cos_t ** 2) * np.sin(phi)], axis=1)
    half_b = abi.make_path_rays(centre + 1.5 * u, -u, 7000 + 31 * k)
    tr = gn.hip_tracer(api, sc, p)
    try:
        first = tr.query_closest(abi.make_rays(half_b["origin"], half_b["dir"]))
        assert (first["object"] == emitter).all() and not (first["hit"] & abi.AOV_HIT_BACKFACE).any(), "every ray of half B hits the emitter first, from outside"
        batches = {"A then B": np.concatenate([half_a, half_b]), "B then A": np.concatenate([half_b, half_a])}
        want, want_nee = {}, {}
        for what, rays in batches.items():
            e = mr.Estimator(pkg, orc, tr, sc.models, sc.triangles, sc.spheres, p)
            want[what] = e.trace(rays)
            b = range(64, 128) if what == "A then B" else range(64)
            assert sorted(e.plain_emission_log) == [(i, 0) for i in b], f"{what}: half B's emitter hits behind no sample"
            a0 = 0 if what == "A then B" else 64
            assert {i for (i, v, *_r) in e.sample_log if v == 0} >= set(range(a0, a0 + 64)) and not any(a0 <= i < a0 + 64 and v == 1 for (i, v, *_r) in e.emission_log)
            want_nee[what] = nr.Estimator(pkg, orc, tr, sc.models, sc.triangles, sc.spheres, p).trace(rays)
    finally:
        tr.close()
    monkeypatch.setenv("RT_GRID", "1")  # read at rt_create: two blocks, one wave
    tr = api.create_tracer(0)
    monkeypatch.delenv("RT_GRID")
    try:
        sc.upload(tr)
        tr.set_params(p)
        got = {what: tr.radiance_trace_mis(rays) for what, rays in batches.items()}
        got_nee = {what: tr.radiance_trace_nee(rays) for what, rays in batches.items()}
    finally:
        tr.close()
    for what in batches:
        gn.assert_records(got[what], want[what], f"rt_mis_trace, {what}")
        assert got[what].tobytes() == want[what].tobytes()
        gn.assert_records(got_nee[what], want_nee[what], f"rt_nee_trace, {what}")
        assert got_nee[what].tobytes() == want_nee[what].tobytes()
    assert got["A then B"][64:].tobytes() == got["B then A"][:64].tobytes(), "half B's records depend on what the lanes did before"
    assert got_nee["A then B"][64:].tobytes() == got_nee["B then A"][:64].tobytes()
    assert got["A then B"][64:]["rgb"].any() and np.isfinite(got["A then B"]["rgb"]).all()
    print(f"{len(keep)} distinct camera rays in half A; half B's records {np.unique(got['A then B'][64:]['rgb'], axis=0).shape[0]} distinct values; "
          f"{time.perf_counter() - t0:.2f} s with the reference's six runs")


# ---------------------------------------------------------------- the rules of emission_weight
_BACK = {}


def back_light_case(pkg, api, orc):
    """near_light_scene's ceiling with the quad light FACING DOWN 4 cm under it: the light's back is towards the ceiling.  An opaque
    model is culled from behind (RC:355: the flag alone decides, no record has a switch for it), so a ceiling vertex's lobe ray goes
    THROUGH the quad; to be hit from behind the quad needs a second, front face towards the ceiling that is no entry's — not this rule.
    What reaches `cl <= 0` is a light whose table normal and whose culling disagree: the model record's worldToLocal is that of the
    quad turned over (facing up), its localToWorld — which alone the light table reads — the quad facing down.  The walk then finds
    the quad from above, the table says it faces down: the sample is rejected (cl <= 0), the lobe ray hits, the emission is added in
    full.  Rays straight up at the ceiling above the quad."""
    if not _BACK:
        M, T = pkg.RayTracingMaterial, pkg.Transform
        ceiling = pkg.Model(pkg.meshes.quad(), M(diffuseCol=(0.8, 0.8, 0.8, 1), specularProbability=0.0), T((0, 3, 0), (-90, 0, 0), (20, 20, 1)), "Ceiling")
        light = pkg.Model(pkg.meshes.quad(), M(diffuseCol=(0, 0, 0, 1), emissionCol=(1, 1, 1, 1), emissionStrength=10.0), T((0, 2.96, 0), (-90, 0, 0), (1, 1, 1)), "DownLight")
        up = T((0, 2.96, 0), (90, 0, 0), (1, 1, 1))
        cam = pkg.Camera(T((3, 1, 0), (0, -90, 0)), fieldOfView=60.0)
        settings = dict(maxBounceCount=2, numRaysPerPixel=1, useSky=False, accumulate=True, bvhQuality=1)
        sc = gn.SceneArrays(api, pkg.scenes.SceneDescription("mis_back_light", 64, 36, 1, settings, cam, [ceiling, light], []))
        sc.models = sc.models.copy()
        sc.models[1]["worldToLocal"] = pkg.manager.matrix_to_abi(up.worldToLocalMatrix)
        p = rr.params_of(sc, api, 64, 36, {})
        k = np.arange(96)
        rays = pkg.abi.make_path_rays(np.stack([-0.4 + 0.8 * (k % 12) / 11, np.full(96, 2.0), -0.4 + 0.8 * (k // 12) / 7], axis=1), np.tile([0.0, 1.0, 0.0], (96, 1)), 300 + 17 * k)
        tr = gn.hip_tracer(api, sc, p)
        try:
            est = mr.Estimator(pkg, orc, tr, sc.models, sc.triangles, sc.spheres, p)
            want = est.trace(rays)
            got = tr.radiance_trace_mis(rays)
        finally:
            tr.close()
        _BACK.update(sc=sc, p=p, rays=rays, est=est, want=want, got=got)
    return _BACK


def test_every_rule_of_emission_weight_is_reached_or_reasoned_unreachable(pkg, api, orc):
    t0 = time.perf_counter()
    for rule, kind, where, why in RULE_TABLE:
        if where is None:
            assert why
            continue
        if where == "mis_back_light":
            b = back_light_case(pkg, api, orc)
            est, what = b["est"], where
            assert b["got"].tobytes() == b["want"].tobytes(), "mis_back_light: rt_mis_trace != the reference"
            assert np.isfinite(b["want"]["rgb"]).all() and b["want"]["rgb"].any()
        else:
            est, what = case(pkg, api, orc, *where)[4], f"{where[0]} bounce={where[1]}"
        rows = [e for e in est.emission_log if e[3] == rule and (kind is None or e[4] == kind)]
        print(f"{rule} ({kind or 'any'}): {len(rows)} rows in {what}")
        assert rows, f"{what} logs no emission under the rule {rule!r} ({kind})"
        assert all(e[2] == 1.0 for e in rows) or rule == mr.WEIGHTED, "every rule but `weighted` adds the emission in full"
    for (name, bounce), c in sorted(_CASES.items(), key=str):
        rules_allowed(c[4], f"{name} bounce={bounce}")
    rules_allowed(back_light_case(pkg, api, orc)["est"], "mis_back_light")
    print(f"{len(_CASES)} cached cases checked against UNREACHABLE; {time.perf_counter() - t0:.2f} s with the reference runs not cached before")


# ---------------------------------------------------------------- 3. the identities
@pytest.mark.parametrize("name", ["config3_bvh", "nee_flat"])
def test_identities_give_rt_radiance_traces_bits(pkg, api, orc, name):
    sc = gn.scene(pkg, api, name)
    models, spheres = sc.stripped()
    for bounce in (None, 1):  # every emission switched off
        p, rays = gn.camera_batch(pkg, api, orc, sc, W, H, bounce)
        if name != "config3_bvh":
            p.useSky = 1  # (light from somewhere; config 3 is a closed room)
        tr = gn.hip_tracer(api, sc, p, models=models, spheres=spheres)
        try:
            assert tr.nee_light_count() == (0, 0)
            plain, got = tr.radiance_trace(rays), tr.radiance_trace_mis(rays)
        finally:
            tr.close()
        assert got.tobytes() == plain.tobytes(), f"{name} without emitters, bounce={p.maxBounceCount}"
        assert (got["rng"] != rays["rng"]).any() and (got["rgb"].any() or name == "config3_bvh")
    p, rays = gn.camera_batch(pkg, api, orc, sc, W, H, 0)  # maxBounceCount = 0, emitters on
    tr = gn.hip_tracer(api, sc, p)
    try:
        assert sum(tr.nee_light_count()) > 0
        plain, got, nee = tr.radiance_trace(rays), tr.radiance_trace_mis(rays), tr.radiance_trace_nee(rays)
    finally:
        tr.close()
    assert got.tobytes() == plain.tobytes(), f"{name} maxBounceCount = 0"
    assert nee.tobytes() != plain.tobytes(), "rt_nee_trace samples at the last vertex: the case would be empty"


@pytest.mark.parametrize("flat", [True, False], ids=["flat", "bvh"])
def test_an_all_mirror_scene_gives_rt_radiance_traces_records(pkg, api, orc, flat):
    sc = gn.scene(pkg, api, "nee_mirrors")
    if not flat:  # the same mirrors around an icosphere mirror: a tree with inner nodes
        key = "mis_mirrors_bvh"
        if key not in gn._SCENES:
            d = nr.build_scene(pkg, "nee_mirrors")
            ball = pkg.Model(pkg.meshes.icosphere(2, radius=1.0), d.models[0].material, pkg.Transform((-2.2, 1.0, 0.4), (0, 0, 0), 0.8), "MirrorBall")
            gn._SCENES[key] = gn.SceneArrays(api, pkg.scenes.SceneDescription(key, 64, 36, 1, d.settings, d.camera, d.models + [ball], d.spheres))
        sc = gn._SCENES[key]
    p, rays = gn.camera_batch(pkg, api, orc, sc, W, H, None)
    tr = gn.hip_tracer(api, sc, p)
    try:
        assert tr.nee_light_count() == (1, 0)
        plain, got = tr.radiance_trace(rays), tr.radiance_trace_mis(rays)
    finally:
        tr.close()
    assert got.tobytes() == plain.tobytes()
    assert got["rgb"].any() and (got["rng"] != rays["rng"]).any()


# ---------------------------------------------------------------- 4. physics, closed form
@pytest.mark.parametrize("offset", [0.7, 2.0])
def test_floor_under_a_spherical_emitter_closed_form(pkg, api, orc, offset):
    """tests/test_gpu_nee.py's floor (rho = 0.8) under an emissive sphere (r = 0.5, 3 above the floor, Le = 10), maxBounceCount = 1, one
    ray straight down `offset` to the side, 2^16 samples: within 5 of its own standard errors + 2^-16 relative of
    rho Le (r / d)^2 cos(theta_c).  At maxBounceCount = 0 the result is exactly 0, where rt_nee_trace's is not."""
    rho, le, r, height = 0.8, 10.0, 0.5, 3.0
    M, S = pkg.RayTracingMaterial, pkg.Sphere
    floor = pkg.Model(pkg.meshes.quad(), M(diffuseCol=(rho, rho, rho, 1), specularProbability=0.0), pkg.Transform((0, 0, 0), (90, 0, 0), (40, 40, 1)), "Floor")
    light = S((0, height, 0), r, M(diffuseCol=(0, 0, 0, 1), emissionCol=(1, 1, 1, 1), emissionStrength=le))
    cam = pkg.Camera(pkg.Transform((0, 1, -6)), fieldOfView=60.0)
    settings = dict(maxBounceCount=1, numRaysPerPixel=1, useSky=False, accumulate=True, bvhQuality=1)
    sc = gn.SceneArrays(api, pkg.scenes.SceneDescription("mis_physics", 64, 36, 1, settings, cam, [floor], [light]))
    p = rr.params_of(sc, api, 64, 36, {})
    assert p.maxBounceCount == 1 and not p.useSky
    ray = pkg.abi.make_path_rays([[offset, 1.0, 0.0]], [[0, -1, 0]], 1)
    tr = gn.hip_tracer(api, sc, p)
    try:
        hit = tr.query_closest(pkg.abi.make_rays(ray["origin"], ray["dir"]))[0]
        mis = gn.chained(tr.radiance_trace_mis, ray, 256, 256)
        p.maxBounceCount = 0
        tr.set_params(p)
        mis0 = gn.chained(tr.radiance_trace_mis, ray, 256, 16)
        nee0 = gn.chained(tr.radiance_trace_nee, ray, 256, 16)
    finally:
        tr.close()
    assert hit["object"] == 1 and np.allclose(hit["normal"], (0, 1, 0), atol=1e-6)
    x = hit["pos"].astype(np.float64) + 0.001 * hit["normal"].astype(np.float64)
    to_c = np.array([0, height, 0]) - x
    d = np.linalg.norm(to_c)
    want = rho * le * (r / d) ** 2 * (to_c[1] / d)
    v = mis[:, 0].astype(np.float64)
    assert len(v) == 1 << 16 and (mis[:, 0] == mis[:, 1]).all() and (mis[:, 0] == mis[:, 2]).all()
    se = np.sqrt(v.var(ddof=1) / len(v))
    print(f"offset {offset}: mis: mean {v.mean():.6f} (closed form {want:.6f}), standard error {se:.3e}, variance {v.var(ddof=1):.6e}, max {v.max():.4f}")
    assert abs(v.mean() - want) <= 5 * se + 2.0 ** -16 * want, (v.mean(), want, se)
    assert not mis0.any(), "maxBounceCount = 0: Trace sees the floor and nothing else"
    assert nee0.any()


def form_factor(x, n, corners):
    """Lambert's formula, float64: the integral of cos / pi over the solid angle of the polygon `corners` seen from x with normal n (the
    polygon lies wholly in n's hemisphere and is not clipped)."""
    v = [(c - x) / np.linalg.norm(c - x) for c in corners]
    total = 0.0
    for a, b in zip(v, v[1:] + v[:1]):
        cr = np.cross(a, b)
        total += np.arccos(np.clip(np.dot(a, b), -1.0, 1.0)) * np.dot(n, cr / np.linalg.norm(cr))
    return abs(total) / (2.0 * np.pi)


_NEAR = {}


def near_light_scene(pkg, api):
    """The case this pass exists for, config 3's ceiling in small: a diffuse ceiling (rho = 0.8, facing down, y = 3) and a 1 x 1 quad
    light (Le = 10, diffuseCol 0) that hangs 4 cm under it.  A quad that faces down cannot be seen by the ceiling above it (cl < 0), so
    the quad hangs vertically in the plane x = 0 and faces +x, like a side of config 3's box light; its top edge is at y = 2.96.  The
    ray goes straight up at the ceiling point (0.04, 3, 0): 4 cm beside the light's plane, 4 cm above its top edge — the vertex sees
    the whole light at grazing angles from a tiny distance."""
    if not _NEAR:
        M, T = pkg.RayTracingMaterial, pkg.Transform
        ceiling = pkg.Model(pkg.meshes.quad(), M(diffuseCol=(0.8, 0.8, 0.8, 1), specularProbability=0.0), T((0, 3, 0), (-90, 0, 0), (20, 20, 1)), "Ceiling")
        m = np.array([[0, 0, -1, 0], [0, 1, 0, 2.46], [1, 0, 0, 0], [0, 0, 0, 1]], dtype=np.float64)  # local -z (the Quad's front) -> world +x
        light = pkg.Model(pkg.meshes.quad(), M(diffuseCol=(0, 0, 0, 1), emissionCol=(1, 1, 1, 1), emissionStrength=10.0), pkg.MatrixTransform(m), "SideLight")
        cam = pkg.Camera(T((3, 1, 0), (0, -90, 0)), fieldOfView=60.0)
        settings = dict(maxBounceCount=1, numRaysPerPixel=1, useSky=False, accumulate=True, bvhQuality=1)
        sc = gn.SceneArrays(api, pkg.scenes.SceneDescription("mis_near_light", 64, 36, 1, settings, cam, [ceiling, light], []))
        p = rr.params_of(sc, api, 64, 36, {})
        assert p.maxBounceCount == 1 and not p.useSky
        ray = pkg.abi.make_path_rays([[0.04, 2.0, 0.0]], [[0, 1, 0]], 1)
        tr = gn.hip_tracer(api, sc, p)
        try:
            hit = tr.query_closest(pkg.abi.make_rays(ray["origin"], ray["dir"]))[0]
            mis = gn.chained(tr.radiance_trace_mis, ray, 256, 256)
            nee = gn.chained(tr.radiance_trace_nee, ray, 256, 256)
        finally:
            tr.close()
        _NEAR.update(sc=sc, p=p, hit=hit, mis=mis, nee=nee)
    return _NEAR


def test_ceiling_point_next_to_a_quad_light_closed_form(pkg, api, orc):
    """rho Le F with F Lambert's polygon form factor of the light seen from x = hit.pos + 0.001 n, in float64: the mean of 2^16 samples
    lies within 5 standard errors + 2^-16 relative."""
    s = near_light_scene(pkg, api)
    hit, mis = s["hit"], s["mis"]
    table = api.light_table_arrays(s["sc"].models, s["sc"].triangles, s["sc"].spheres)
    assert table["n_triangle_entries"] == 2 and np.allclose(table["entries"]["ng"], (1, 0, 0), atol=1e-6), "the light faces +x"
    assert hit["object"] == 0 and np.allclose(hit["normal"], (0, -1, 0), atol=1e-6) and abs(float(hit["pos"][1]) - 3.0) < 1e-5
    x = hit["pos"].astype(np.float64) + 0.001 * hit["normal"].astype(np.float64)
    n = hit["normal"].astype(np.float64)
    F_ = 0.0
    for e in table["entries"]:
        a = e["a"].astype(np.float64)
        corners = [a, a + e["e1"].astype(np.float64), a + e["e2"].astype(np.float64)]
        assert all(np.dot(c - x, n) > 0 for c in corners) and all(c[1] <= 2.96 + 1e-6 for c in corners)
        F_ += form_factor(x, n, corners)
    want = 0.8 * 10.0 * F_
    v = mis[:, 0].astype(np.float64)
    assert len(v) == 1 << 16
    se = np.sqrt(v.var(ddof=1) / len(v))
    w = s["nee"][:, 0].astype(np.float64)
    print(f"form factor {F_:.6f}: mis mean {v.mean():.6f} (closed form {want:.6f}), standard error {se:.3e}, variance {v.var(ddof=1):.4e}, max {v.max():.3f}; "
          f"nee mean {w.mean():.6f}, variance {w.var(ddof=1):.4e}, max {w.max():.3f}")
    assert 0.05 < F_ < 0.5
    assert abs(v.mean() - want) <= 5 * se + 2.0 ** -16 * want, (v.mean(), want, se)


# ---------------------------------------------------------------- 5. the bound
def test_every_record_keeps_the_headers_bound_where_nee_does_not(pkg, api, orc):
    """rgb <= 2 (maxBounceCount + 1) max(Le) + the sky's bound (0: no sky), componentwise, for each of the 2^16 records of the ceiling
    point; the same batch through rt_nee_trace has records above it."""
    s = near_light_scene(pkg, api)
    bound = 2.0 * (s["p"].maxBounceCount + 1) * 10.0
    assert s["sc"].models["material"]["diffuseCol"].max() <= 1.0 and s["sc"].models["material"]["specularCol"].max() <= 1.0
    assert np.isfinite(s["mis"]).all() and (s["mis"] >= 0).all()
    print(f"bound {bound}: mis max {s['mis'].max():.4f}; nee max {s['nee'].max():.2f}, {int((s['nee'].max(axis=1) > bound).sum())} of {len(s['nee'])} nee records above it")
    assert (s["mis"] <= bound).all(), f"{int((s['mis'] > bound).any(axis=1).sum())} records above the bound, the largest {s['mis'].max()}"
    assert (s["nee"] > bound).any(), "rt_nee_trace stays under the bound here: the case shows nothing"


# ---------------------------------------------------------------- 6. the same expectation
@pytest.mark.parametrize("bounce", [1, None], ids=["bounce_1", "bounce_default"])
@pytest.mark.parametrize("name", ["nee_flat", "config3_bvh", "nee_glass"])
def test_same_expectation_as_plain_radiance(pkg, api, orc, name, bounce):
    """2^20 paths each way over 24 x 16 camera rays, fixed seeds, as tests/test_gpu_nee.py's: per colour channel the float64 means of
    rt_mis_trace and rt_radiance_trace differ by at most 5 combined standard errors — at maxBounceCount 1 too, where rt_nee_trace's
    expectation is not Trace's."""
    sc = gn.scene(pkg, api, name)
    p, cam = gn.camera_batch(pkg, api, orc, sc, 24, 16, bounce)
    reps = -(-(1 << 20) // len(cam))
    rays = np.tile(cam, reps)
    rays["rng"] = (np.arange(len(rays), dtype=np.uint64) * 2654435761 + 977) % (1 << 32)
    assert len(rays) >= 1 << 20
    tr = gn.hip_tracer(api, sc, p)
    try:
        mis = tr.radiance_trace_mis(rays)["rgb"].astype(np.float64)
        plain = tr.radiance_trace(rays)["rgb"].astype(np.float64)
        nee = tr.radiance_trace_nee(rays)["rgb"].astype(np.float64)
    finally:
        tr.close()
    assert np.isfinite(mis).all() and np.isfinite(plain).all()
    n = len(rays)
    for c in range(3):
        m1, m2 = mis[:, c].mean(), plain[:, c].mean()
        s1, s2 = np.sqrt(mis[:, c].var(ddof=1) / n), np.sqrt(plain[:, c].var(ddof=1) / n)
        print(f"{name} bounce={p.maxBounceCount} channel {c}: mis {m1:.6f} +- {s1:.2e}, plain {m2:.6f} +- {s2:.2e}, difference {abs(m1 - m2) / np.hypot(s1, s2):.2f} combined "
              f"standard errors; variance ratio mis / plain {mis[:, c].var() / plain[:, c].var():.4f}, mis / nee {mis[:, c].var() / nee[:, c].var():.4f} (nee mean {nee[:, c].mean():.6f})")
        assert m1 > 0 and m2 > 0
        assert abs(m1 - m2) <= 5 * np.hypot(s1, s2), (name, c, m1, m2, s1, s2)


# ---------------------------------------------------------------- 7. the side-pass manners
def test_device_form_launches_held_back_frames_first_like_a_flushes_row(pkg, api, orc, monkeypatch):
    """What tests/test_gpu_held_back.py checks for the call's `flushes` rows (tests/flush_table.py: rt_mis_trace and its device_form case,
    which tests/test_flush_table.py finds through the descriptor's context member), here with the records of the pass compared as well: with RT_HOLD_BACK=1 and three frames held, none is pending after the
    call, and the final image, the last frame and the frame counter are those of an eager twin context (RT_COALESCE=0)."""
    abi = pkg.abi
    results = []
    for env in ("RT_HOLD_BACK", "RT_COALESCE"):
        monkeypatch.setenv(env, "1" if env == "RT_HOLD_BACK" else "0")
        tr = api.create_tracer(0)
        monkeypatch.delenv(env)
        try:
            mgr = pkg.scenes.get(2).make_manager(tr, api, 64, 36)
            mgr.OnEnable(renderSeed=3)
            n = 70
            rays = np.repeat(abi.make_path_rays([[0.0, 0.05, 0.0]], [[0, -1, 0]], 9), n)
            rays["origin"][:, 0] += np.arange(n) * F(0.002)
            rays["rng"] = np.arange(n) + 100
            d_rays, d_out = DevBuf(rays.nbytes).upload(rays), DevBuf(n * 16)
            mgr.RenderFrames(2)
            before = tr.radiance_trace_mis(rays)
            for _ in range(3):
                mgr.RenderFrame()
            if env == "RT_HOLD_BACK":
                assert held_at(tr, "test_gpu_mis: rt_mis_trace (device form) behind rt_render_frame", True) == 3
            else:
                assert tr.pending_frames() == 0
            tr.radiance_trace_mis_buffers(d_rays.ptr, n, d_out.ptr)
            assert tr.pending_frames() == 0, "the call left frames held back"
            mgr.RenderFrames(2)
            tr.synchronize()
            assert d_out.download(abi.RADIANCE_DTYPE).tobytes() == before.tobytes()
            results.append((tr.read_accumulated().tobytes(), tr.read_frame().tobytes(), tr.frame()))
            d_rays.free(), d_out.free()
        finally:
            tr.close()
    assert results[0] == results[1] and results[0][2] == 8


def test_device_form_sees_updates_and_the_rebuilt_map(pkg, api, orc):
    """Behind rt_update_spheres (no synchronise in between) the pass sees the new emitter, and switching a model's emission off and on
    is seen: each time the records are those of a context that was given the changed scene from the start."""
    abi = pkg.abi
    sc, p, rays, want, est = case(pkg, api, orc, "config3_bvh", None)
    names = [m.name for m in sc.desc.models]
    light, cube = names.index("Light"), names.index("OpaqueRoundedCube")
    n = len(rays)
    d_rays, d_out = DevBuf(n * 32).upload(rays), DevBuf(n * 16)

    def device(tr):
        tr.radiance_trace_mis_buffers(d_rays.ptr, n, d_out.ptr)
        tr.synchronize()
        return d_out.download(abi.RADIANCE_DTYPE)

    def fresh(**arrays):
        t = gn.hip_tracer(api, sc, p, **arrays)
        try:
            return t.radiance_trace_mis(rays)
        finally:
            t.close()
    tr = gn.hip_tracer(api, sc, p)
    try:
        assert device(tr).tobytes() == want.tobytes()
        off = sc.models.copy()
        off["material"]["emissionStrength"][light] = 0
        tr.update_models(off)
        dark = device(tr)
        assert dark.tobytes() == tr.radiance_trace(rays).tobytes() and not dark["rgb"].any()
        on = off.copy()
        on["material"]["emissionCol"][cube] = (1, 0.5, 0.2, 1)
        on["material"]["emissionStrength"][cube] = 4.0
        tr.update_models(on)
        lit = device(tr)  # the pass itself rebuilds the table and the map: the cube's triangles now have entries, the light's none
        assert lit.tobytes() == fresh(models=on).tobytes() and lit["rgb"].any() and lit.tobytes() != want.tobytes()
        tr.update_models(sc.models)
        assert device(tr).tobytes() == want.tobytes()
    finally:
        tr.close()
        d_rays.free(), d_out.free()
    # spheres: scene 2, every sphere put out and one lit
    tr = api.create_tracer(0)
    try:
        mgr = pkg.scenes.get(2).make_manager(tr, api, 64, 36)
        mgr.OnEnable(renderSeed=3)
        spheres = mgr._pack_spheres()
        m = 70
        rays2 = np.repeat(abi.make_path_rays([[0.0, 0.05, 0.0]], [[0, -1, 0]], 9), m)
        rays2["origin"][:, 0] += np.arange(m) * F(0.002)
        rays2["rng"] = np.arange(m) + 100
        d_rays, d_out = DevBuf(rays2.nbytes).upload(rays2), DevBuf(m * 16)
        before = tr.radiance_trace_mis(rays2)
        changed = spheres.copy()
        changed["material"]["emissionStrength"][:] = 0
        changed["material"]["emissionCol"][0] = (0.5, 0.25, 0.125, 1)
        changed["material"]["emissionStrength"][0] = 2.0
        changed["material"]["flag"][0] = 0
        tr.update_spheres(changed)
        tr.radiance_trace_mis_buffers(d_rays.ptr, m, d_out.ptr)  # no synchronise in between
        tr.synchronize()
        seen = d_out.download(abi.RADIANCE_DTYPE)
        other = api.create_tracer(0)
        try:
            data = mgr.CreateAllMeshData(mgr.models)
            other.upload_scene(data["meshInfo"], data["triangles"], data["nodes"], changed)
            other.set_params(mgr.params())
            assert seen.tobytes() == other.radiance_trace_mis(rays2).tobytes(), "the pass behind the update != a context that was given the updated scene"
        finally:
            other.close()
        assert seen.tobytes() != before.tobytes()
        d_rays.free(), d_out.free()
    finally:
        tr.close()


def test_mixed_calls_of_the_three_estimators_and_frames_leave_no_trace(pkg, api, orc):
    """Behind frames, moments and a tile selection: everything a caller can read (targets, counters, the frame counter, the moments,
    the tile list) is the same before and after host- and device-form calls of the three estimators in a row, each device-form
    pass wrote its own estimator's records, and the closing rt_synchronize — which reports every pass's watchdog word — is RT_OK."""
    sc, p, rays, want, est = case(pkg, api, orc, "config3_bvh", None)
    n = len(rays)
    bufs = (DevBuf(n * 32).upload(rays), DevBuf(n * 16), DevBuf(n * 16), DevBuf(n * 16))
    tr = api.create_tracer(0)
    try:
        tr.enable_stats(True)
        mgr = pkg.scenes.get(3).make_manager(tr, api, 64, 40)
        mgr.OnEnable(renderSeed=5)
        mgr.RenderFrames(4)
        tr.variance_update()
        mgr.RenderFrames(4)
        tr.variance_update()
        tr.adaptive_select(tr.adaptive_params(threshold=0.01, minFrames=0))
        mgr.RenderFrame()
        others = (tr.radiance_trace(rays).tobytes(), tr.radiance_trace_nee(rays).tobytes())
        before = tq.snapshot(tr)
        assert before["counters"]["segments"] > 0
        got = tr.radiance_trace_mis(rays)
        tr.radiance_trace_mis_buffers(bufs[0].ptr, n, bufs[1].ptr)
        tr.radiance_trace_nee_buffers(bufs[0].ptr, n, bufs[2].ptr)
        tr.radiance_trace_buffers(bufs[0].ptr, n, bufs[3].ptr)
        tr.radiance_trace_mis_buffers(bufs[0].ptr, n, bufs[1].ptr)
        assert tr.radiance_trace_mis(rays[:0]).shape == (0,)
        tr.synchronize()  # (would report any pass's watchdog word)
        after = tq.snapshot(tr)
        assert before == after, [k for k in before if before[k] != after[k]]
        assert bufs[1].download(np.uint8).tobytes() == got.tobytes() and got["rgb"].any()
        assert (bufs[3].download(np.uint8).tobytes(), bufs[2].download(np.uint8).tobytes()) == others
        assert others == (tr.radiance_trace(rays).tobytes(), tr.radiance_trace_nee(rays).tobytes())
    finally:
        tr.close()
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
    tr = api.create_tracer(0)

    def call(form, r, k, o, **kw):
        b = tr._mis_batch(form, r, k, o)
        for f, v in kw.items():
            setattr(b, f, v)
        return api.mis_trace(C.byref(b))

    def host(r, k, o, **kw):
        return call(abi.MIS_HOST, r, k, o, **kw)

    def dev(r, k, o, **kw):
        return call(abi.MIS_DEVICE, r, k, o, **kw)
    try:
        tr.set_params(p)  # parameters, no scene
        assert host(rays.ctypes.data, n, out.ctypes.data) == state and b"rt_upload_scene" in api.last_error(tr.h)
        assert dev(d_rays.ptr, n, d_out.ptr) == state and b"rt_upload_scene" in api.last_error(tr.h)
        tr.close()
        tr = sc.upload(api.create_tracer(0))  # a scene, no parameters
        assert host(rays.ctypes.data, n, out.ctypes.data) == state and b"rt_set_params" in api.last_error(tr.h)
        assert dev(d_rays.ptr, n, d_out.ptr) == state and b"rt_set_params" in api.last_error(tr.h)
        tr.set_params(p)
        # the descriptor, with a context: the text is the context's
        assert host(rays.ctypes.data, n, out.ctypes.data, reserved=1) == bad and b"reserved" in api.last_error(tr.h)
        assert host(rays.ctypes.data, n, out.ctypes.data, memory=2) == bad and b"memory" in api.last_error(tr.h)
        assert host(rays.ctypes.data, n, out.ctypes.data, struct_size=36) == bad
        assert host(rays.ctypes.data, -1, out.ctypes.data) == bad
        assert host(rays.ctypes.data, (1 << 26) + 1, out.ctypes.data) == bad
        assert host(None, n, out.ctypes.data) == bad
        assert host(rays.ctypes.data, n, None) == bad
        assert host(rays.ctypes.data, 2, rays.ctypes.data + 32) == bad  # the output overlaps the rays
        assert host(rays.ctypes.data, 0, out.ctypes.data) == ok and host(None, 0, None) == ok
        assert dev(d_rays.ptr, -1, d_out.ptr) == bad
        assert dev(d_rays.ptr, (1 << 26) + 1, d_out.ptr) == bad
        assert dev(None, n, d_out.ptr) == bad
        assert dev(d_rays.ptr, n, None) == bad
        assert dev(rays.ctypes.data, n, d_out.ptr) == bad        # host memory
        assert dev(d_rays.ptr, n, out.ctypes.data) == bad
        assert dev(d_rays.ptr + 4, n - 1, d_out.ptr) == bad      # misaligned
        assert dev(d_rays.ptr, n - 1, d_out.ptr + 4) == bad
        assert dev(d_rays.ptr + 32, n, d_out.ptr) == bad         # runs past the allocation
        assert dev(d_rays.ptr, n, d_out.ptr + 16) == bad
        assert dev(d_rays.ptr, 2, d_rays.ptr + 32) == bad        # the output overlaps the rays
        assert dev(d_rays.ptr, 0, d_out.ptr) == ok and dev(None, 0, None) == ok
        assert not out.view(np.uint32).any(), "a refused call wrote records"
        assert host(rays.ctypes.data, n, out.ctypes.data) == ok
        assert dev(d_rays.ptr, n, d_out.ptr) == ok
        tr.synchronize()
        assert out.tobytes() == want[:n].tobytes(), "after the errors"
        assert d_out.download(np.uint8).tobytes() == out.tobytes()
    finally:
        tr.close()
        d_rays.free(), d_out.free()


def test_more_entries_than_the_cap_is_a_scene_error_of_this_call_only(pkg, api, orc):
    """tests/test_gpu_nee.py's 65 emissive models over one mesh of 2^16 triangles: 2^16 entries past RT_NEE_MAX_LIGHTS.  Both forms
    refuse with RT_ERR_SCENE and say why, every time; nothing is enqueued or written; the scene stays usable."""
    abi = pkg.abi
    M, T = pkg.RayTracingMaterial, pkg.Transform
    mesh = gn.grid_mesh(pkg)
    lit = dict(diffuseCol=(0, 0, 0, 1), emissionCol=(1, 0.9, 0.8, 1), emissionStrength=3.0)
    models = [pkg.Model(mesh, M(**lit), T((0, 0.05 * k, 3 + 0.02 * k), (0, 0, 0), (2.0, 1.0, 1)), f"Panel{k}") for k in range(65)]
    models.append(nr._floor(pkg))
    cam = pkg.Camera(T((0, 1, -4)), fieldOfView=60.0)
    settings = dict(maxBounceCount=2, numRaysPerPixel=1, useSky=False, accumulate=True, bvhQuality=1)
    sc = gn.SceneArrays(api, pkg.scenes.SceneDescription("mis_cap", 64, 36, 1, settings, cam, models, []))
    p, rays = gn.camera_batch(pkg, api, orc, sc, 16, 8, None)
    n = len(rays)
    out = np.zeros(n, dtype=abi.RADIANCE_DTYPE)
    d_rays, d_out = DevBuf(n * 32).upload(rays), DevBuf(n * 16)
    tr = gn.hip_tracer(api, sc, p)
    try:
        for _ in range(2):
            for b in (tr._mis_batch(abi.MIS_HOST, rays.ctypes.data, n, out.ctypes.data), tr._mis_batch(abi.MIS_DEVICE, d_rays.ptr, n, d_out.ptr)):
                assert api.mis_trace(C.byref(b)) == abi.RT_ERR_SCENE
                assert api.last_error(tr.h).startswith(b"rt_mis_trace: ") and b"RT_NEE_MAX_LIGHTS" in api.last_error(tr.h)
        tr.synchronize()
        assert not out.view(np.uint32).any() and not d_out.download(np.uint32).any(), "a refused call wrote records"
        plain = tr.radiance_trace(rays)
        assert plain["rgb"].any()
    finally:
        tr.close()
        d_rays.free(), d_out.free()


def test_watchdog_fails_the_pass_not_the_context(pkg, api, orc, monkeypatch):
    """RT_TRAV_LIMIT=4 (the forced step limit of tests/test_gpu_nee.py: a software counter, nothing can hang): the walks of the pass are
    cut short.  The host form says so when it returns, the device form at the next rt_synchronize or rt_mis_trace, once; the frames
    rendered before stay readable; the other estimators report their own words only."""
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
        sc.upload(tr)
        monkeypatch.delenv("RT_TRAV_LIMIT")

        def reported(e, call, *holds):
            msg = str(e.value)
            assert e.value.status == abi.RT_ERR_HIP and "watchdog" in msg, msg
            assert msg.startswith(f"rt status {abi.RT_ERR_HIP}: {call}: "), msg
            for text in holds:
                assert text in msg, (text, msg)
            return msg
        family = "in the pass of a device-form rt_mis_trace call"
        with pytest.raises(abi.RtError) as e:
            tr.radiance_trace_mis(rays)
        reported(e, "rt_mis_trace", "in this pass", "the records are not valid")
        tr.radiance_trace_mis_buffers(bufs[0].ptr, n, bufs[1].ptr)  # enqueued: RT_OK
        with pytest.raises(abi.RtError) as e:
            tr.synchronize()
        reported(e, "rt_synchronize", family)
        tr.synchronize()  # reported once
        tr.radiance_trace_mis_buffers(bufs[0].ptr, n, bufs[1].ptr)
        with pytest.raises(abi.RtError) as e:  # the next rt_mis_trace reports it if it comes first ...
            tr.radiance_trace_mis_buffers(bufs[0].ptr, n, bufs[1].ptr)
        reported(e, "rt_mis_trace", family)
        tr.synchronize()  # ... once (and the call that reported enqueued nothing)
        tr.radiance_trace_mis_buffers(bufs[0].ptr, n, bufs[1].ptr)
        with pytest.raises(abi.RtError) as e:  # the NEE pass neither reports it nor is failed by it
            tr.radiance_trace_nee(rays)
        assert "mis" not in reported(e, "rt_nee_trace", "in this pass")
        with pytest.raises(abi.RtError) as e:
            tr.synchronize()
        reported(e, "rt_synchronize", family)
        tr.synchronize()
        assert tr.frame() == 3
        assert tr.read_accumulated().tobytes() == image  # RT_OK: the context's watchdog word was not set
        sc.upload(tr)
        tr.set_params(p)
        assert tr.radiance_trace_mis(rays).tobytes() == want.tobytes(), "after the re-upload"
    finally:
        tr.close()
        for b in bufs:
            b.free()


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
    mgr.InitBVH()
    mgr.SetShaderParams()
    n = 1000
    o = rng.normal(size=(n, 3)); o = 2.5 * o / np.linalg.norm(o, axis=1, keepdims=True) + [0, 2, 0]
    d = rng.uniform(-2, 2, (n, 3)) + [0, 1, 0] - o
    rays = abi.make_path_rays(o, d, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))
    host = tr.radiance_trace_mis(rays)
    assert host["rgb"].any() and (host["rng"] != rays["rng"]).any()
    assert host.tobytes() != tr.radiance_trace(rays).tobytes() and host.tobytes() != tr.radiance_trace_nee(rays).tobytes()
    t_rays = torch.from_numpy(rays.view(np.uint32).reshape(n, 8).copy().view(np.int32)).to("cuda:0")
    t_out = torch.full((n, 4), 0x7fc00001, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    tr.radiance_trace_mis_buffers(t_rays.data_ptr(), n, t_out.data_ptr())
    tr.synchronize()
    assert t_out.cpu().numpy().tobytes() == host.tobytes(), "tensor != host form (config %d)" % cfg
    s = torch.cuda.Stream()
    tr.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        t2 = torch.zeros((n, 4), dtype=torch.int32, device="cuda:0")
        s.synchronize()
        tr.radiance_trace_mis_buffers(t_rays.data_ptr(), n, t2.data_ptr())
        copy = t2.clone()
    s.synchronize()
    assert copy.cpu().numpy().tobytes() == host.tobytes(), "stream order (config %d)" % cfg
    tr.set_stream(None)
    tr.synchronize()
    tr.close()
print("MIS_TORCH_OK")
"""


def test_device_form_into_torch_tensors(pkg, api):
    """The device form on torch tensors' data_ptr()s == the host form, and in the order of a torch stream given to rt_set_stream.  In a
    child process that imports torch first, so that the library shares torch's HIP runtime."""
    p = subprocess.run([sys.executable, "-c", _TORCH_CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "MIS_TORCH_OK" in p.stdout, "rc=%d\n%s\n%s" % (p.returncode, p.stdout[-3000:], p.stderr[-3000:])


@pytest.mark.parametrize("layout", gn.LAYOUTS)
@pytest.mark.parametrize("name", ["config3_bvh", "nee_instances"])
def test_every_device_layout_gives_the_references_records(pkg, api, orc, monkeypatch, capfd, name, layout):
    """As tests/test_gpu_nee.py's: the reverse lookup names a triangle by hit_triangle(), which under `dense` divides the unit by 3 and
    under every other layout reads the unit -> triangle map; a wrong index would weight the wrong emission, or none."""
    monkeypatch.delenv("RT_LAYOUT", raising=False)
    sc, p, rays, want, est = case(pkg, api, orc, name, None)
    used = api.layout_arrays(sc.models, sc.triangles, sc.nodes, layout)["used"]
    assert gn.without_cache(used) == gn.without_cache(layout), f"asked for {layout}, the scene is laid out as {used}"
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
        got = tr.radiance_trace_mis(rays)
    finally:
        tr.close()
    assert [gn.without_cache(r) for r in reported] == [gn.without_cache(used)], f"asked for {layout}: the upload reports {reported}, rt_debug_layout {used}"
    gn.assert_records(got, want, f"{name}, RT_LAYOUT={layout}")
    assert weighted(est, "triangle"), "no weighted emission on a triangle: the lookup was not reached"
