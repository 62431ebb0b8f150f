"""The FLAT trace kernel's table of per-launch ray-origin constants (ray-tracing_amd/csrc/rt_primary.h) on the GPU.

A wave whose active lanes are all fresh camera rays of a launch without defocus reads |o|^2, c.o, o - c, the origin in model space and
o' - A from a table the host filled once per launch instead of computing them per lane: same fp32 operations on the same values, so the
image and the exact counters must not move by a bit.  Every case here is rendered FOUR ways — table on / RT_PRIMARY=0, as pooled
workgroups (RT_POOL_MIN_ITEMS=0: also at these small sizes) / as single waves (RT_POOL=0) — by the shipped and by the STATS
instantiation, and each of the eight images is compared bit for bit with the CPU oracle's, the STATS counters with the oracle's, and
the audits of the conservative pre-tests (filter_violations) with 0.  The oracle renders each case once.

The cases are the ones in which a stale, misplaced or wrongly enabled table would show: fused launches, a camera move, sphere and model
updates between frames, defocus (table off), sphere counts 1 / 3 (the pair's tail) / 33 (over the cap: off), more models or triangles
than the caps (off), a 12-triangle leaf next to a quad (within the caps), maxBounceCount = 0 (every intersection is a camera ray's)."""
import numpy as np
import pytest

from gpu_support import KEYS, bits, environment

pytestmark = pytest.mark.gpu
# RT_PRIMARY and RT_POOL_MIN_ITEMS are read when a context is made, RT_POOL when a scene is uploaded
ENV = ("RT_PRIMARY", "RT_POOL", "RT_POOL_MIN_ITEMS")
WAYS = [("table, pooled", {"RT_PRIMARY": "1", "RT_POOL_MIN_ITEMS": "0"}), ("no table, pooled", {"RT_PRIMARY": "0", "RT_POOL_MIN_ITEMS": "0"}),
        ("table, single waves", {"RT_PRIMARY": "1", "RT_POOL": "0"}), ("no table, single waves", {"RT_PRIMARY": "0", "RT_POOL": "0"})]


def check(pkg, api, orc, drive, table=True):
    """drive(lib, tracer) renders the case and returns nothing; the tracer holds the result.  table: whether the case's last launch
    carries the table switched on when RT_PRIMARY allows it (rt_debug_primary_table) — a table that is never on would pass every
    comparison below and lose the speed-up unnoticed"""
    c = orc.create_tracer(8)
    drive(orc, c)
    want, wantCounters = c.read_accumulated(), c.counters()
    c.close()
    images = {}
    for name, env in WAYS:
        with environment(env, ENV):
            for stats in (False, True):
                g = api.create_tracer(0)
                g.enable_stats(stats)
                drive(api, g)
                got, counters = g.read_accumulated(), g.counters()
                violations = g.phase_profile()["filter_violations"][0] if stats else 0
                on = g.primary_table()
                g.close()
                assert on == (1 if table and env["RT_PRIMARY"] == "1" else 0), f"{name}, stats={stats}: rt_debug_primary_table() = {on}"
                assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), f"{name}, stats={stats}: image differs from the oracle's"
                assert counters["segments"] == wantCounters["segments"] and counters["pixelFrames"] == wantCounters["pixelFrames"], (name, stats)
                if stats:
                    assert [counters[k] for k in KEYS] == [wantCounters[k] for k in KEYS], name
                    assert violations == 0, name
        images[name] = got
    assert np.array_equal(bits(images["table, pooled"]), bits(images["no table, pooled"]))
    assert np.array_equal(bits(images["table, single waves"]), bits(images["no table, single waves"]))


def scene_driver(pkg, cfg, w, h, steps, change_scene=None, tweak=None):
    """A case: scene `cfg` (changed by change_scene(scene)), settings changed by tweak(manager), then steps(manager, tracer)"""
    def drive(lib, tr):
        sc = pkg.scenes.get(cfg)
        if change_scene:
            change_scene(sc)
        mgr = sc.make_manager(tr, lib, w, h)
        if tweak:
            tweak(mgr)
        mgr.OnEnable(renderSeed=1)
        steps(mgr, tr)
    return drive


def frames(n):
    return lambda mgr, tr: mgr.RenderFrames(n)


def test_config2_at_the_goldens_size(pkg, api, orc):
    check(pkg, api, orc, scene_driver(pkg, 2, 96, 54, frames(2)))


def test_config1_spheres_only(pkg, api, orc):
    check(pkg, api, orc, scene_driver(pkg, 1, 64, 64, frames(2)))


def test_fused_launch_of_five_frames(pkg, api, orc):
    check(pkg, api, orc, scene_driver(pkg, 2, 64, 36, frames(5)))


def test_camera_move_between_frames(pkg, api, orc):
    def steps(mgr, tr):
        mgr.RenderFrame()
        t = mgr.camera.transform
        mgr.camera.transform = type(t)(position=(1.25, 3.5, -7.0), euler=(18, -9, 0))
        try:
            mgr.RenderFrame()
            mgr.RenderFrames(2)
        finally:
            mgr.camera.transform = t   # (the scene description's camera object is shared)
    check(pkg, api, orc, scene_driver(pkg, 2, 64, 36, steps))


def test_sphere_and_model_updates_between_frames(pkg, api, orc):
    def steps(mgr, tr):
        mgr.RenderFrames(2)
        mgr.spheres[3].centre = (mgr.spheres[3].centre[0] + 0.75, mgr.spheres[3].centre[1] + 0.5, mgr.spheres[3].centre[2] - 1.0)
        mgr.spheres[7].radius = mgr.spheres[7].radius * 1.5
        tr.update_spheres(mgr._pack_spheres())
        t = mgr.models[0].transform
        mgr.models[0].transform = type(t)(position=(0.5, -0.25, 1.0), euler=(84, 10, 0), scale=(40, 40, 1))  # InitFrame -> rt_update_models
        mgr.RenderFrames(2)
        mgr.RenderFrame()
    check(pkg, api, orc, scene_driver(pkg, 2, 64, 36, steps))


def test_defocus_keeps_the_table_off(pkg, api, orc):
    def tweak(mgr):
        mgr.defocusStrength = 120.0
        mgr.focusDistance = 7.0
    check(pkg, api, orc, scene_driver(pkg, 2, 64, 36, frames(2), tweak=tweak), table=False)


def _spheres(pkg, n):
    """n spheres on a grid over the ground, a third of them glass"""
    mod = pkg.manager
    rnd = pkg.meshes._lcg(7)
    out = []
    for i in range(n):
        r = 0.25 + 0.35 * rnd()
        kw = dict(diffuseCol=(0.3 + 0.6 * rnd(), 0.3 + 0.6 * rnd(), 0.3 + 0.6 * rnd(), 1.0))
        if i % 3 == 2:
            kw = dict(flag=pkg.abi.MATERIAL_GLASS, ior=1.5, smoothness=1.0, specularProbability=1.0, absorption=(0.2, 0.4, 0.1, 1), absorptionMultiplier=0.6)
        out.append(mod.Sphere(((i % 7 - 3) * 1.4 + 0.3 * rnd(), r, (i // 7 - 2) * 1.5 + 0.3 * rnd()), r, mod.RayTracingMaterial(**kw)))
    return out


@pytest.mark.parametrize("n", [1, 3, 33])
def test_sphere_counts(pkg, api, orc, n):
    """1 and 3: the second half of the last pair record is a copy; 33: a second block of the pre-test, over the table's cap"""
    def change(sc):
        sc.spheres = _spheres(pkg, n)
    check(pkg, api, orc, scene_driver(pkg, 2, 64, 36, frames(2), change_scene=change), table=n <= 32)


def _boxes(pkg, sc, n_cubes, n_quads):
    mod = pkg.manager
    cube, quad = pkg.meshes.cube(), pkg.meshes.quad()
    sc.spheres = sc.spheres[:3]
    for i in range(n_cubes):
        sc.models.append(mod.Model(cube, mod.RayTracingMaterial(diffuseCol=(0.8, 0.5, 0.2, 1)), mod.Transform(position=(-2.0 + 2.5 * i, 0.6, 1.0 + i), euler=(0, 30 * i + 15, 0), scale=(1.2, 1.2, 1.2))))
    for i in range(n_quads):
        sc.models.append(mod.Model(quad, mod.RayTracingMaterial(diffuseCol=(0.2, 0.5, 0.9, 1)), mod.Transform(position=(-3.0 + 2.0 * i, 1.0, 4.0), euler=(0, 20 * i, 0), scale=(1.5, 2.0, 1))))


def _one_leaf_per_mesh(pkg):
    def tweak(mgr):
        mgr.bvhQuality = pkg.abi.BVH_QUALITY_DISABLED   # the whole mesh in its root leaf -> a FLAT scene
    return tweak


@pytest.mark.parametrize("cubes,quads", [(1, 0), (2, 0), (0, 4)])
def test_leaf_sizes_and_the_caps(pkg, api, orc, cubes, quads):
    """ground + one cube: 2 + 12 triangles in two models, within the caps; + two cubes: 26 triangles, over the triangle cap; + four
    quads: five models, over the model cap"""
    check(pkg, api, orc, scene_driver(pkg, 2, 64, 36, frames(2), change_scene=lambda sc: _boxes(pkg, sc, cubes, quads), tweak=_one_leaf_per_mesh(pkg)), table=(cubes, quads) == (1, 0))


def test_no_bounces_every_intersection_is_a_camera_rays(pkg, api, orc):
    def tweak(mgr):
        mgr.maxBounceCount = 0
    check(pkg, api, orc, scene_driver(pkg, 2, 64, 36, frames(2), tweak=tweak))
