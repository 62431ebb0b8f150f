"""The FLAT trace kernel's per-tile triangle candidates (tile_tri_mask of ray-tracing_amd/csrc/rt_tile_cand.h) on the GPU.

The per-tile table holds a second mask per 8 x 8 tile: the root-leaf triangles the tile's camera rays can be accepted by.  A wave whose
active lanes are all fresh camera rays tests only the triangles some lane wants and skips a model none of whose triangles is wanted.  The
exact test is unchanged and a triangle is skipped only where it could not be accepted, so the image and the exact counters must not move
by a bit.  Every case here is rendered EIGHT ways — triangle masks on / RT_TILE_TRI=0, as pooled workgroups (RT_POOL_MIN_ITEMS=0: also at
these small sizes) / as single waves (RT_POOL=0), by the shipped and by the STATS instantiation — and each image is compared bit for bit
with ONE render of the CPU oracle, the segment counters (and, in the STATS build, all exact counters) with the oracle's, the audit of
the filters (filter_violations: in the STATS build every triangle a lane's mask dropped goes through the exact test) with 0, and
rt_debug_tile_tri / rt_debug_tile_cand with what the caps and the switch say: masks that silently stayed off would pass everything else.

The sequences are the ones in which a stale table would show: a model moved between frames, a camera move, single frames (two parts, one
per stream) alternating with fused launches (which alternate between the streams themselves).  On config 2 the STATS phase profile must
count fewer `tri` wave executions with the masks than without: masks that clear nothing would pass everything else too."""
import numpy as np
import pytest

from gpu_support import KEYS, bits, environment

pytestmark = pytest.mark.gpu
# RT_TILE_TRI, RT_TILE_CAND and RT_POOL_MIN_ITEMS are read when a context is made, RT_POOL when a scene is uploaded
ENV = ("RT_TILE_TRI", "RT_TILE_CAND", "RT_PRIMARY", "RT_POOL", "RT_POOL_MIN_ITEMS")
WAYS = [("masks, pooled", {"RT_TILE_TRI": "1", "RT_POOL_MIN_ITEMS": "0"}), ("no masks, pooled", {"RT_TILE_TRI": "0", "RT_POOL_MIN_ITEMS": "0"}),
        ("masks, single waves", {"RT_TILE_TRI": "1", "RT_POOL": "0"}), ("no masks, single waves", {"RT_TILE_TRI": "0", "RT_POOL": "0"})]


def check(pkg, api, orc, drive, table=True, part=None):
    """drive(lib, tracer) renders the case; the tracer holds the result.  table: whether the case's last launch is within the caps.
    part = (strip_rows, index, count): the GPU contexts render that part of the image and are compared with its rows of the oracle's
    whole image; their counters (a part's share, which the oracle does not have) must then agree among the eight ways.
    Returns the STATS build's `tri` wave executions per way."""
    c = orc.create_tracer(8)
    drive(orc, c)
    want, wantCounters = c.read_accumulated(), c.counters()
    c.close()
    first = None
    triExec = {}
    for name, env in WAYS:
        with environment(env, ENV):
            for stats in (False, True):
                g = api.create_tracer(0)
                if part:
                    g.set_partition(*part)
                g.enable_stats(stats)
                drive(api, g)
                got, counters = g.read_accumulated(), g.counters()
                prof = g.phase_profile() if stats else None
                tri, cand, primary = g.tile_tri(), g.tile_cand(), g.primary_table()
                g.close()
                what = f"{name}, stats={stats}"
                assert primary == (1 if table else 0), f"{what}: rt_debug_primary_table() = {primary}"
                assert cand == (1 if table else 0), f"{what}: rt_debug_tile_cand() = {cand}"
                assert tri == (1 if table and env["RT_TILE_TRI"] == "1" else 0), f"{what}: rt_debug_tile_tri() = {tri}"
                if part:
                    rows = pkg.dist.global_rows_of(part[1], part[2], want.shape[0], part[0])
                    assert np.array_equal(bits(got), bits(want[rows])), f"{what}: image differs from the oracle's rows"
                    first = first or counters
                    for k in ("segments", "pixelFrames"):
                        assert counters[k] == first[k], (what, k)
                else:
                    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), f"{what}: image differs from the oracle's"
                    assert counters["segments"] == wantCounters["segments"] and counters["pixelFrames"] == wantCounters["pixelFrames"], what
                    if stats:
                        assert [counters[k] for k in KEYS] == [wantCounters[k] for k in KEYS], what
                if stats:
                    assert prof["filter_violations"][0] == 0, what
                    triExec[name] = prof["tri"][0]
    return triExec


def scene_driver(pkg, cfg, w, h, steps, change_scene=None, tweak=None):
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


@pytest.mark.parametrize("cfg,w,h", [(2, 96, 54), (2, 37, 23), (1, 64, 64)])
def test_config_scenes(pkg, api, orc, cfg, w, h):
    tri = check(pkg, api, orc, scene_driver(pkg, cfg, w, h, frames(3)))
    print(f"config {cfg} at {w}x{h}: tri wave executions per way: {tri}")
    if cfg == 2:   # (config 1 has no triangles)
        assert tri["masks, pooled"] < tri["no masks, pooled"]
        assert tri["masks, single waves"] < tri["no masks, single waves"]


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


@pytest.mark.parametrize("cubes,quads", [(1, 0), (0, 3), (2, 0), (0, 4)])
def test_leaf_sizes_and_the_caps(pkg, api, orc, cubes, quads):
    """ground + one cube: 14 triangles in two models, a model most tiles skip whole; ground + three quads: four models, at the model cap;
    + two cubes: 26 triangles, over the triangle cap; + four quads: five models, over the model cap.  Over a cap the table of ray-origin
    constants is off (rt_primary.h), the per-tile table rides on it, and so both of its halves stay off, as the sphere half always did."""
    within = (cubes, quads) in ((1, 0), (0, 3))
    tri = check(pkg, api, orc, scene_driver(pkg, 2, 64, 36, frames(2), change_scene=lambda sc: _boxes(pkg, sc, cubes, quads), tweak=_one_leaf_per_mesh(pkg)), table=within)
    if within:
        assert tri["masks, pooled"] < tri["no masks, pooled"]


def test_defocus_keeps_both_halves_off(pkg, api, orc):
    def tweak(mgr):
        mgr.defocusStrength = 120.0
        mgr.focusDistance = 7.0
    check(pkg, api, orc, scene_driver(pkg, 2, 64, 36, frames(2), tweak=tweak), table=False)


def test_cull_off_and_camera_under_the_ground(pkg, api, orc):
    """a glass ground (RC:355: no backface culling) seen from below: every ground tile's rays are accepted from the back"""
    def change(sc):
        sc.models[0].material.flag = pkg.abi.MATERIAL_GLASS
        t = sc.camera.transform
        sc.camera.transform = type(t)(position=(0, -2.0, -8.8), euler=(-12, 0, 0))
    check(pkg, api, orc, scene_driver(pkg, 2, 64, 36, frames(2), change_scene=change))


def test_strip_partition_two_of_three(pkg, api, orc):
    """local tile rows are not global rows: part 1 of 3 at 96x54 owns rows 8-15 and 32-39"""
    check(pkg, api, orc, scene_driver(pkg, 2, 96, 54, frames(3)), part=(8, 1, 3))


def test_a_model_and_the_camera_moved_between_frames(pkg, api, orc):
    """masks made for the old ground or the old camera would drop the ground from tiles it now covers"""
    def steps(mgr, tr):
        mgr.RenderFrames(2)
        t = mgr.models[0].transform
        mgr.models[0].transform = type(t)(position=(3.0, 0.8, 2.0), euler=(70, 25, 0), scale=(-9, 6, 1))  # InitFrame -> rt_update_models; mirrored
        mgr.RenderFrames(2)
        c = mgr.camera.transform
        mgr.camera.transform = type(c)(position=(1.25, 3.5, -7.0), euler=(18, -9, 0))
        try:
            mgr.RenderFrame()
            mgr.RenderFrames(2)
        finally:
            mgr.camera.transform = c   # (the scene description's camera object is shared)
    check(pkg, api, orc, scene_driver(pkg, 2, 64, 36, steps))


def test_single_frames_and_fused_launches_on_both_streams(pkg, api, orc):
    """a single frame runs as two parts, one per stream; fused launches alternate between the streams: each stream's table is filled
    once, by whichever launch first needs it, and read by all of them"""
    def steps(mgr, tr):
        idle = getattr(tr, "synchronize", lambda: None)   # (an idle GPU starts a single frame at once instead of holding it back)
        mgr.RenderFrame()
        idle()
        mgr.RenderFrames(17)
        idle()
        mgr.RenderFrame()
        idle()
        mgr.RenderFrames(2)
    check(pkg, api, orc, scene_driver(pkg, 2, 64, 36, steps))
