"""The BVH traversal stack at its exact bound, on every kernel that takes its LDS layout from the scene's tree height.

tests/deep_trees.py makes trees in which most camera rays push at EVERY level: a launch with `max_height` stack rows has its last row
written by them, and the row behind it is pixel-field row 0 (the trace and cost kernels' bookkeeping, the query and radiance kernels' ray
index), or — behind the pixel fields — the candidate-mask summary of the scenes with more than 64 models.  tests/test_deep_trees.py
asserts, without a GPU, that the heights are exact and that the rays are there.  Everything here is compared bit for bit with the oracle
(oracle/rt_oracle.cpp, a stack of 64), and — up to the height the reference's driver lets reach its `int stack[32]`, 30 — with the
reference's text compiled as C++ where it travelled:

  a. rt_render_frame(s): combs of height 1, 2, 30, 31 and 32, inner child on either side, tied, from behind, with a shared subtree — as
     single-wave workgroups, as the default groups, with a 16-record cache and with two further group sizes; the launch's own report
     (RT_DEBUG_LAUNCH) must name exactly H stack entries;
  b. comb(32) beside a cube, and inside scenes of 65 and 97 models (the > 64-model instantiation), in both model orders;
  c. rt_render_cost, rt_render_aov, rt_render_aov_centre, rt_query_closest / _occluded, rt_radiance_trace and rt_debug_intersect on
     comb(32), comb_tied(32) and the 65-model scene, the query batches with a whole wave of witness rays;
  d. a refused upload (33 levels) leaves the context rendering its previous scene;
  e. the 40-triangle mesh that the builders take to depth 32: rt_build_bvh_gpu(_batch) against the host builder, and rendered;
  f. rt_nee_trace, the one kernel with two run-to-completion walks per wave iteration through one stack region: emissive, diffuse combs
     of height 1, 31 and 32, the tied comb and the 65-model scene, a wave's worth of identical witness rays whose shadow ray AND next
     segment hold H entries, against tests/nee_reference.py bit for bit (in order, reversed, as prefixes, the buffer form with guard
     bytes), the coverage asserted from that reference's ray logs;
  g. rt_mis_trace, the same two walks with two things of its own behind them: the bounce row (in the > 64-model instantiation the LDS
     word behind the candidate-mask extension, which decides whether a vertex samples — on the 65-model scene it lies directly behind a
     32-entry stack) and the reverse lookup entry(hit object, hit triangle) on a leaf at level H.  The batch of (f), its witness chosen
     by tests/mis_reference.py, bit for bit against that reference; rt_debug_light_map against the reference's map."""
import ctypes as C
import re
import time

import numpy as np
import pytest

import aov_support as ta
import cost_view_support as tc
import deep_trees as dt
import mis_reference as mr
import motion_reference as mref
import nee_reference as nr
import radiance_reference as rr
import query_support as tq
from cost_view_support import orc_log  # noqa: F401  (fixture)
from deep_trees import CATCHER_POINT, CATCHER_Z, CONE_SCALE, cone_camera, cone_mesh, launches
from gpu_support import KEYS, DevBuf, bits

pytestmark = pytest.mark.gpu
F = np.float32
F3 = C.c_float * 3
W, H = dt.W, dt.H_IMG
FRAME = 3
WITNESS = (H // 2, W // 2)  # the pixel whose ray fills a whole wave of the query batches

_SCENES, _ORACLE, _REF = {}, {}, {}


# ---------------------------------------------------------------- scenes
def crowd(pkg, n, seed=3):
    """n small models between the camera and the comb and beside it: cubes, rounded cubes and quads, every fourth glass, every ninth
    emitting (tests/fuzz_scenes.py::crowded_overflow_scene's mix, placed for deep_trees.camera)"""
    rng = np.random.default_rng(seed)
    M, T = pkg.RayTracingMaterial, pkg.Transform
    meshes = [pkg.meshes.cube(), pkg.meshes.rounded_cube(3), pkg.meshes.quad()]
    return [pkg.Model(meshes[i % 3], M(flag=int(i % 4 == 3) * 2, diffuseCol=tuple(rng.uniform(0.2, 1, 3)) + (1,), ior=1.4,
                                       emissionStrength=float(i % 9 == 0) * 3.0, emissionCol=(1, 0.9, 0.7, 1)),
                      T((float(rng.uniform(-2.5, 2.5)), float(rng.uniform(-1.6, 1.6)), float(rng.uniform(2.0, 3.6))), tuple(rng.uniform(0, 360, 3)),
                        float(rng.uniform(0.12, 0.35))))
            for i in range(n)]


def nee_scene(pkg, name):
    """comb<H>alternate-emissive | tied32-emissive | crowd65_first-emissive: the tree as model 0, untransformed, opaque, diffuse AND
    emitting — every leaf an entry of rt_nee's light table, and a surface whose vertices sample that table; behind it (the crowd
    scene) the first 62 models of crowd65_first, of which seven emit; then a small diffuse quad behind the camera that faces the comb,
    the catcher — a path that starts towards it has its first vertex there, and its shadow ray and its next segment go up the comb
    like camera rays; last a dark quad at z = 2 that stands in the way of some of those shadow rays (the only thing in front of leaf 0,
    which in comb(1) is the only leaf that faces the catcher: without it no shadow ray of that scene could be blocked).  Both quads
    come after the comb: its walk starts with nothing hit, as deep_trees.occupancy assumes.  65 models in the crowd scene."""
    abi, M, T = pkg.abi, pkg.RayTracingMaterial, pkg.Transform
    base = name[:-len("-emissive")]
    m = re.fullmatch(r"comb(\d+)alternate", base)
    if m:
        tree = dt.comb(abi, int(m.group(1)), "alternate")
    elif base == "tied32":
        tree = dt.comb_tied(abi, 32)
    else:
        assert base == "crowd65_first", name
        tree = dt.comb(abi, 32, "alternate")
    lit = M(diffuseCol=(0.7, 0.6, 0.5, 1), specularProbability=0.0, emissionCol=(1, 0.8, 0.5, 1), emissionStrength=2.0)
    matte = M(diffuseCol=(0.8, 0.8, 0.8, 1), specularProbability=0.0)
    catcher = pkg.Model(pkg.meshes.quad(), matte, T((0, 0, CATCHER_Z), (0, 180, 0), (0.6, 0.6, 1)), "Catcher")  # (the Quad's front is local -z)
    blocker = pkg.Model(pkg.meshes.quad(), matte, T((-0.8, 0.5, 2.0), (0, 0, 0), (1.5, 1.5, 1)), "Blocker")
    models = [pkg.Model(dt.HandMesh(base, *tree), lit, T())] + (crowd(pkg, 62) if base == "crowd65_first" else []) + [catcher, blocker]
    assert base != "crowd65_first" or len(models) == 65
    return dt.description(pkg, name, models, maxBounceCount=2)  # (two bounces: the reference is Python)


def scene(pkg, name):
    """comb<H><form>[-diffuse] | tied32 | behind32 | shared32 | cube_first | cube_last | crowd<N>_first | crowd<N>_last | nee_scene's"""
    if name in _SCENES:
        return _SCENES[name]
    if name.endswith("-emissive"):
        _SCENES[name] = nee_scene(pkg, name)
        return _SCENES[name]
    abi = pkg.abi
    cam = None
    m = re.fullmatch(r"comb(\d+)(A|B|alternate)(-diffuse)?", name)
    if m:
        mesh = dt.HandMesh(name, *dt.comb(abi, int(m.group(1)), m.group(2)))
        models = dt.tree_models(pkg, mesh, "diffuse" if m.group(3) else "glass")
    elif name == "tied32":
        models = dt.tree_models(pkg, dt.HandMesh(name, *dt.comb_tied(abi, 32)))
    elif name == "behind32":
        models, cam = dt.tree_models(pkg, dt.HandMesh(name, *dt.comb_behind(abi, 32))), dt.camera(pkg, behind=True)
    elif name == "shared32":
        models = dt.tree_models(pkg, dt.HandMesh(name, *dt.shared(abi, 16, 16)))
    else:
        comb = pkg.Model(dt.HandMesh("comb32", *dt.comb(abi, 32, "alternate")), dt.materials(pkg)["glass"], pkg.Transform())
        kind, order = name.split("_")
        if kind == "cube":
            others = [pkg.Model(pkg.meshes.cube(), dt.materials(pkg)["diffuse"], pkg.Transform((0.8, -0.5, 3.0), (20, 30, 0), 0.9))]
        else:
            others = crowd(pkg, int(kind[5:]) - 1)
        models = [comb] + others if order == "first" else others[::-1] + [comb]
    _SCENES[name] = dt.description(pkg, name, models, cam)
    return _SCENES[name]


def height_of(name):
    m = re.match(r"comb(\d+)", name)
    return int(m.group(1)) if m else 32


def render(lib, tr, desc, stats=False, seed=9):
    """Two frames, the first with the pixel-centre rays the witness shares were computed for, the second jittered: both render targets,
    the seven counters, the STATS build's filter audit and cache count.  lib: what builds the ordinary meshes and the view parameters."""
    if stats:
        tr.enable_stats(True)
    mgr = desc.make_manager(tr, lib)
    mgr.OnEnable(renderSeed=seed)
    mgr.RenderFrame()
    mgr.divergeStrength = 0.7
    mgr.RenderFrame()
    c = tr.counters()
    prof = tr.phase_profile() if stats else None
    out = dict(acc=tr.read_accumulated(), frame=tr.read_frame(), counters=[c[k] for k in KEYS],
               viol=prof["filter_violations"][0] if stats else 0, hot=prof["inner_from_lds_cache"][0] if stats else None)
    tr.close()
    return out


def oracle_render(pkg, orc, name):
    if name not in _ORACLE:
        _ORACLE[name] = render(orc, orc.create_tracer(8), scene(pkg, name))
    return _ORACLE[name]


def ref_lib():
    """The reference's text compiled as C++ (oracle/_ref/libref.so), or None where it did not travel"""
    if "lib" not in _REF:
        import __graft_entry__ as graft
        _REF["lib"] = graft.load_ref()
    return _REF["lib"]


def same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_render(got, want, what, stats):
    assert same(got["acc"], want["acc"]), f"{what}: accumulated image differs in {int((got['acc'] != want['acc']).any(axis=-1).sum())} pixels"
    assert same(got["frame"], want["frame"]), f"{what}: last frame differs in {int((got['frame'] != want['frame']).any(axis=-1).sum())} pixels"
    if stats:
        assert got["counters"] == want["counters"], (what, dict(zip(KEYS, got["counters"])), dict(zip(KEYS, want["counters"])))
        assert got["viol"] == 0, what
    else:  # the shipped instantiation counts segments and pixel frames only
        for k in ("segments", "pixelFrames"):
            assert got["counters"][KEYS.index(k)] == want["counters"][KEYS.index(k)], (what, k)


# ---------------------------------------------------------------- a. the trace kernels
SHAPES = [("single", {"RT_HOT_KB": "0"}), ("default", {}), ("cache16", {"RT_HOT_KB": "1"}), ("groups8", {"RT_WAVES_PER_GROUP": "8"}),
          ("groups4", {"RT_WAVES_PER_GROUP": "4"})]
TRACE_SCENES = ([f"comb{h}{form}" + ("-diffuse" if form == "B" else "") for h in (1, 2, 30, 31, 32) for form in ("A", "B", "alternate")] +
                ["comb32A-diffuse", "comb32B", "comb32alternate-diffuse", "tied32", "behind32", "shared32"])


@pytest.mark.parametrize("name", TRACE_SCENES)
def test_trace_kernels_fill_the_last_stack_row(pkg, api, orc, name, monkeypatch, capfd):
    desc, height = scene(pkg, name), height_of(name)
    want = oracle_render(pkg, orc, name)
    assert want["counters"][KEYS.index("innerSteps")] > 0 and np.isfinite(want["acc"]).all() and want["acc"][..., :3].any()
    t0 = time.perf_counter()
    monkeypatch.setenv("RT_DEBUG_LAUNCH", "1")
    monkeypatch.delenv("RT_LAYOUT", raising=False)
    seen = {}
    for shape, env in SHAPES:
        for k in ("RT_HOT_KB", "RT_WAVES_PER_GROUP"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        capfd.readouterr()
        for stats in (False, True):
            got = render(api, api.create_tracer(0), desc, stats)
            assert_render(got, want, f"{name}, {shape}, {'stats' if stats else 'shipped'} build", stats)
        reported = launches(capfd)
        assert reported and {r[1] for r in reported} == {height}, (name, shape, reported)
        # what rt_launch_plan.h's arithmetic gives a wave: (stack + 4 pixel fields) x 64 dwords; the rest of a workgroup's LDS is the cache
        for variant, stack, lds, threads, records in reported:
            assert lds == records * 64 + (threads // 64) * (stack + 4) * 256, (name, shape, reported)
        seen[shape] = sorted({(r[3], r[4]) for r in reported})
        if shape == "single":
            assert seen[shape] == [(64, 0)], (name, seen)
        if shape == "cache16" and height == 30:  # 16 records of 30 pairs: a walk alternates between the LDS copy and global memory
            assert seen[shape][0][1] == 16 and 0 < got["hot"] < want["counters"][KEYS.index("innerSteps")], (name, seen, got["hot"])
        if shape == "default" and height <= 30:
            assert seen[shape][0][0] > 64 and got["hot"] > 0, (name, seen, got["hot"])
    line = f"{name}: height {height}, stack entries reported {height}; (threads, cache records) per shape {seen}"
    ref = ref_lib() if height <= 31 else None  # never at 32: the reference's int stack[32] stands at H + 1 entries
    if ref is not None:
        try:
            # (the reference's dispatcher has no builder and no view parameters: the oracle's serve the manager)
            got = render(orc, ref.create_tracer(4), desc)
        except pkg.abi.RtError as e:
            # the reference's driver (oracle/ref_driver.h) counts the root as a level and lets at most 31 reach the text: height 31 is its 32nd
            assert height == 31 and "int stack[32]" in str(e), (name, str(e))
            line += "; reference text: refused by its driver's guard"
        else:
            assert height <= 30
            assert same(got["acc"], want["acc"]) and same(got["frame"], want["frame"]), f"{name}: the reference's text differs from the oracle"
            for k in ("segments", "innerSteps", "triTests"):  # its own two statistics (RC:254, RC:271) and the segments
                assert got["counters"][KEYS.index(k)] == want["counters"][KEYS.index(k)], (name, k)
            line += "; reference text: same bits"
    else:
        line += "; reference text: not compared" + (" (never at 32)" if height == 32 else " (not here)")
    print(f"{line}; {time.perf_counter() - t0:.1f} s")


# ---------------------------------------------------------------- b. mixed heights and more than 64 models
@pytest.mark.parametrize("kind", ["cube", "crowd65", "crowd97"])
def test_comb_32_beside_other_models_in_both_orders(pkg, api, orc, kind, monkeypatch, capfd):
    monkeypatch.setenv("RT_DEBUG_LAUNCH", "1")
    t0 = time.perf_counter()
    lines = []  # (printed at the end: reading the launch reports takes what was printed before with it)
    for order in ("first", "last"):
        name = f"{kind}_{order}"
        desc = scene(pkg, name)
        n_models = len(desc.models)
        want = oracle_render(pkg, orc, name)
        assert want["counters"][KEYS.index("modelVisits")] == want["counters"][KEYS.index("segments")] * n_models
        for shape, env in (("default", {}), ("cache", {"RT_LAYOUT": "pre,arena,cache"}), ("single", {"RT_HOT_KB": "0"})):
            for k in ("RT_HOT_KB", "RT_LAYOUT"):
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            capfd.readouterr()
            for stats in (False, True):
                got = render(api, api.create_tracer(0), desc, stats)
                assert_render(got, want, f"{name}, {shape}, {'stats' if stats else 'shipped'} build", stats)
            assert got["counters"][KEYS.index("modelVisits")] == got["counters"][KEYS.index("segments")] * n_models
            reported = launches(capfd)
            assert reported and {r[1] for r in reported} == {32}, (name, shape, reported)
            ext = 0 if n_models <= 64 else (n_models - 63 + 31) // 32
            for variant, stack, lds, threads, records in reported:
                assert (variant in (4, 5, 10, 11)) == (n_models > 64), (name, reported)  # the > 64-model instantiations
                assert lds == records * 64 + (threads // 64) * (32 + 4 + (2 + ext if ext else 0)) * 256, (name, shape, reported)
            if kind == "crowd65" and shape == "cache":  # the one deep shape with a cache: 8 waves around 16 records (tests/test_launch_plan.py)
                assert sorted({(r[3], r[4]) for r in reported}) == [(512, 16)] and got["hot"] > 0, (name, reported, got["hot"])
            lines.append(f"{name}, {shape}: {n_models} models, stack entries reported 32, (variant, threads, cache records) {sorted({(r[0], r[3], r[4]) for r in reported})}")
    print("\n".join(lines + [f"{kind}: {time.perf_counter() - t0:.1f} s, the oracle's renders included"]))


# ---------------------------------------------------------------- c. the other kernels
SIDE_SCENES = ["comb32alternate", "tied32", "crowd65_first"]


@pytest.fixture()
def named_scenes(pkg, monkeypatch):
    """tests/test_gpu_aov.py's and tests/test_gpu_cost_view.py's helpers take a scene by name through their scene_of"""
    monkeypatch.setattr(ta, "scene_of", scene)
    monkeypatch.setattr(tc, "scene_of", scene)


def witness_batch(pkg, api, orc, name, p):
    """130 of the image's restated camera rays (frame FRAME, no jitter): 33 pixels, the witness pixel 64 times over — a whole wave on the
    last stack row, whatever block the batch is cut into — and 33 more.  Returns the pixel indices, origins, directions, generator states."""
    origins, dirs, states = rr.camera_rays(orc, p, W, H, FRAME)
    flat = np.arange(W * H)
    wit = WITNESS[0] * W + WITNESS[1]
    idx = np.concatenate([flat[5::11][:33], np.full(64, wit), flat[2::11][:33]])
    assert len(idx) == 130
    o, d, s = origins.reshape(-1, 3)[idx], dirs.reshape(-1, 3)[idx], states.reshape(-1)[idx]
    mesh = scene(pkg, name).models[0].Mesh  # model 0: the tree, untransformed
    occ, _ = dt.occupancy(mesh.nodes, o[40], d[40], mesh.tris, cull=False)
    assert occ == 32, (name, occ)
    return idx, o, d, s


@pytest.mark.parametrize("name", SIDE_SCENES)
def test_cost_view_of_deep_trees(pkg, api, orc_log, named_scenes, name):  # noqa: F811
    t0 = time.perf_counter()
    for frame in (1, 2):
        got = tc.gpu_cost(pkg, api, name, W, H, frame)
        want = tc.oracle_cost(pkg, orc_log, name, W, H, frame)
        tc.assert_cost_equal(got, want, f"{name}, frame {frame}")
        # a witness ray's first segment: 32 inner steps down model 0's comb at the least
        assert want[WITNESS][4] >= 32, want[WITNESS].tolist()
    print(f"{name}: rt_render_cost, {time.perf_counter() - t0:.1f} s")


@pytest.mark.parametrize("name", SIDE_SCENES)
def test_aov_passes_of_deep_trees(pkg, api, orc, named_scenes, name):
    tr, ot = api.create_tracer(0), orc.create_tracer(1)
    try:
        su = ta.Setup(pkg, api, tr, name, W, H)
        so = ta.Setup(pkg, orc, ot, name, W, H)
        for which in ("rt_render_aov", "rt_render_aov_centre"):
            if which == "rt_render_aov":
                su.mgr.divergeStrength = so.mgr.divergeStrength = 0.7  # jittered rays for the frame's pass, the centre pass has none
                p = su.params(FRAME)
                tr.set_params(p)
                aov = tr.render_aov(FRAME)
                origins, dirs = ta.camera_rays(orc, p, W, H, FRAME)
            else:
                p = su.params(1)
                aov = tr.render_aov_centre()
                origins, dirs = mref.centre_rays(orc, p, W, H)
            assert aov.shape == (H, W) and aov.dtype == pkg.abi.AOV_DTYPE
            want = ta.oracle_records(pkg, orc, ot, so, p, origins, dirs, aov["object"])
            want["triangle"] = aov["triangle"]  # (checked below, as tests/test_gpu_aov.py checks it)
            ta.assert_records_equal(aov, want, f"{name}: {which}")
            hit = aov["hit"] & 3
            assert np.array_equal(aov["object"] >= 0, hit != 0) and (hit != 0).mean() > 0.5
            assert ta.check_triangles(orc, so, aov, origins, dirs) > W * H // 4, "model 0 (untransformed) must be what most pixels see"
            dbg = tr.debug_intersect(origins.reshape(-1, 3), dirs.reshape(-1, 3)).reshape(H, W, 10)
            assert dbg[..., 2].view(np.uint32).tolist() == aov["dst"].view(np.uint32).tolist(), which
            assert dbg[..., 3:6].view(np.uint32).tolist() == aov["normal"].view(np.uint32).tolist(), which
    finally:
        tr.close()
        ot.close()


@pytest.mark.parametrize("name", SIDE_SCENES)
def test_ray_queries_and_radiance_with_a_wave_of_witness_rays(pkg, api, orc, named_scenes, name):
    abi = pkg.abi
    tr, ot = api.create_tracer(0), orc.create_tracer(1)
    try:
        su = ta.Setup(pkg, api, tr, name, W, H)
        ta.Setup(pkg, orc, ot, name, W, H)
        p = su.params(FRAME)
        tr.set_params(p)
        ot.set_params(p)
        idx, o, d, states = witness_batch(pkg, api, orc, name, p)
        n = len(idx)
        want10 = tq.oracle_hits(orc, ot, o, d)
        hit = want10[:, 0] != 0
        assert hit[33:97].all() and hit.sum() >= 100
        dbg = tr.debug_intersect(o, d)
        guard = 64
        for what, order in (("in order", np.arange(n)), ("reversed", np.arange(n)[::-1])):
            rays = abi.make_rays(o[order], d[order])
            # ---- closest hit: every field against the oracle's function and against rt_debug_intersect
            got = tr.query_closest(rays)
            tq.assert_same_records(got, tq.records_from_oracle(pkg, None, want10[order], got["object"], got["triangle"]), f"{name}, {what}")
            assert not got["reserved"].any()
            assert (got["object"][hit[order]] >= 0).all() and (got["triangle"][hit[order]] >= 0).all()
            assert bits(dbg[order, 2]).tolist() == bits(got["dst"]).tolist()
            assert bits(dbg[order, 3:6]).tolist() == bits(got["normal"]).tolist() and bits(dbg[order, 6:9]).tolist() == bits(got["pos"]).tolist()
            assert np.array_equal(dbg[order, 0] != 0, (got["hit"] & 3) != 0) and np.array_equal(dbg[order, 1] != 0, (got["hit"] & 0x100) != 0)
            # the 64 witness slots hold one and the same record
            w64 = got[33:97] if what == "in order" else got[n - 97:n - 33]
            assert len({r.tobytes() for r in w64}) == 1
            # ---- the buffer form, with guard words behind the last record
            d_rays, d_hits = DevBuf(n * 32).upload(rays), DevBuf(n * 48 + guard, fill=0xa5)
            tr.query_closest_buffers(d_rays.ptr, n, d_hits.ptr)
            tr.synchronize()
            raw = d_hits.download(np.uint8)
            assert raw[:n * 48].tobytes() == got.tobytes() and (raw[n * 48:] == 0xa5).all(), (name, what)
            # ---- occlusion below tmax = +inf, d, d / 2
            dist = np.where(hit, want10[:, 2], F(1)).astype(F)[order]
            for tname, tmax in (("+inf", np.full(n, np.inf, dtype=F)), ("d", dist), ("d / 2", dist / F(2))):
                occ = tr.query_occluded(abi.make_rays(o[order], d[order], tmax=tmax))
                wanted = (hit[order] & (want10[order, 2] < tmax)).astype(np.uint32)
                assert np.array_equal(occ, wanted), (name, what, tname, np.argwhere(occ != wanted).ravel()[:5])
                d_occ = DevBuf(n * 4 + guard, fill=0xa5)
                d_rays.upload(abi.make_rays(o[order], d[order], tmax=tmax))
                tr.query_occluded_buffers(d_rays.ptr, n, d_occ.ptr)
                tr.synchronize()
                raw = d_occ.download(np.uint8)
                assert raw[:n * 4].tobytes() == occ.tobytes() and (raw[n * 4:] == 0xa5).all(), (name, what, tname)
                d_occ.free()
                if tname == "+inf":
                    assert occ[hit[order]].all()
                else:
                    assert not occ.any()  # nothing lies strictly below the closest hit's distance, or half of it
            d_rays.free(), d_hits.free()
        # ---- rt_radiance_trace: the same rays with their generator states against oracle_trace_pixel
        want_rgb = np.zeros((n, 3), dtype=F)
        o3 = F3()
        for k, i in enumerate(idx):
            orc.trace_pixel(ot.h, int(i % W), int(i // W), FRAME, o3)
            want_rgb[k] = o3[:]
        assert np.isfinite(want_rgb).all() and want_rgb.any()
        for what, order in (("in order", np.arange(n)), ("reversed", np.arange(n)[::-1])):
            got = tr.radiance_trace(abi.make_path_rays(o[order], d[order], states[order]))
            bad = np.argwhere((rr.bits(got["rgb"]) != rr.bits(want_rgb[order])).any(axis=1)).ravel()
            assert not len(bad), f"{name}, rt_radiance_trace {what}: {len(bad)} of {n} rays differ; first is ray {bad[0]}: got {got['rgb'][bad[0]]}, want {want_rgb[order][bad[0]]}"
            assert (got["rng"] != states[order]).any()
    finally:
        tr.close()
        ot.close()


# ---------------------------------------------------------------- d. a refused upload
def test_refused_upload_of_33_levels_leaves_the_context_usable(pkg, api, orc):
    desc = scene(pkg, "comb32alternate")
    bad = dt.one_model(pkg, *dt.comb(pkg.abi, 33))
    frames = []
    for lib, tr in ((api, api.create_tracer(0)), (orc, orc.create_tracer(8))):
        mgr = desc.make_manager(tr, lib)
        mgr.OnEnable(renderSeed=4)
        mgr.RenderFrame()
        first = tr.read_accumulated().copy()
        if lib is api:
            with pytest.raises(pkg.abi.RtError) as e:
                tr.upload_scene(*bad, None)
            assert e.value.status == pkg.abi.RT_ERR_SCENE and "BVH depth 33 > 32" in str(e.value), str(e.value)
        mgr.RenderFrame()
        frames.append((first, tr.read_accumulated(), tr.read_frame(), tr.counters()["segments"]))
        tr.close()
    (a1, a2, af, sa), (b1, b2, bf, sb) = frames
    assert same(a1, b1) and same(a2, b2) and same(af, bf) and sa == sb and not same(a1, a2)


# ---------------------------------------------------------------- e. the builder's depth-32 mesh
def cone_scene(pkg, where):
    v, nrm, idx = cone_mesh()
    cone = pkg.meshes.Mesh(v, nrm, idx, "cone")
    mats = dt.materials(pkg)
    models = [pkg.Model(cone, mats["glass"], pkg.Transform((0, 0, 0), (0, 0, 0), CONE_SCALE)),
              pkg.Model(cone, mats["diffuse"], pkg.Transform((0.3, 0.4, 1.0), (0, 0, 25), CONE_SCALE)),
              pkg.Model(pkg.meshes.cube(), mats["emitter"], pkg.Transform((3.0, -2.5, 0.5), (0, 30, 0), 1.5))]
    return pkg.scenes.SceneDescription("cone_" + where, W, H, 2, dict(dt.SETTINGS), cone_camera(pkg, where), models, [])


def test_gpu_builder_takes_the_cone_to_depth_32_and_the_scene_renders_the_same_bits(pkg, api, orc, monkeypatch, capfd):
    v, nrm, idx = cone_mesh()
    nodes, tris, stats = api.build_bvh_arrays(v, nrm, idx, 1)
    assert stats["leafDepthMax"] == 32
    stats.pop("timeMs")
    n2, t2, s2 = api.build_bvh_arrays_gpu(v, nrm, idx, 1)
    s2.pop("timeMs")
    assert n2.tobytes() == nodes.tobytes() and t2.tobytes() == tris.tobytes() and s2 == stats
    # between two ordinary meshes in one batch
    before, after = pkg.meshes.rounded_cube(4), pkg.meshes.icosphere(2, 1.0, 5)
    nb, tb, per = api.build_bvh_arrays_gpu_batch([(m.vertices, m.normals, m.triangles) for m in (before, pkg.meshes.Mesh(v, nrm, idx), after)], 1)
    host = [api.build_bvh_arrays(m.vertices, m.normals, m.triangles, 1) for m in (before, after)]
    host.insert(1, (nodes, tris, dict(stats)))
    ends = [per[k + 1][:2] if k + 1 < len(per) else (len(nb), len(tb)) for k in range(3)]
    for k, ((n_off, t_off, s), (hn, ht, hs), (n_end, t_end)) in enumerate(zip(per, host, ends)):
        s.pop("timeMs"), hs.pop("timeMs", None)
        assert nb[n_off:n_end].tobytes() == hn.tobytes() and tb[t_off:t_end].tobytes() == ht.tobytes() and s == hs, k
    # rendered: the trees built on the GPU, against the oracle with its own builder
    monkeypatch.setenv("RT_DEBUG_LAUNCH", "1")
    lines = []
    for where in ("apex", "outside"):
        desc = cone_scene(pkg, where)
        want = render(orc, orc.create_tracer(8), desc)
        assert np.isfinite(want["acc"]).all() and want["acc"][..., :3].any()
        capfd.readouterr()
        for stats_on in (False, True):
            tr = api.create_tracer(0)
            if stats_on:
                tr.enable_stats(True)
            mgr = desc.make_manager(tr, api)
            mgr.bvhOnGpu = True
            mgr.OnEnable(renderSeed=9)
            mgr.RenderFrame()
            mgr.divergeStrength = 0.7
            mgr.RenderFrame()
            c = tr.counters()
            got = dict(acc=tr.read_accumulated(), frame=tr.read_frame(), counters=[c[k] for k in KEYS],
                       viol=tr.phase_profile()["filter_violations"][0] if stats_on else 0)
            tr.close()
            assert_render(got, want, f"cone from {where}, {'stats' if stats_on else 'shipped'} build", stats_on)
        reported = launches(capfd)
        assert reported and {r[1] for r in reported} == {32}, reported
        lines.append(f"cone from {where}: stack entries reported 32, {want['counters'][KEYS.index('innerSteps')]} inner steps")
    print("\n".join(lines))


# ---------------------------------------------------------------- f. rt_nee: two walks per wave iteration through one stack region
NEE_SCENES = ["comb1alternate-emissive", "comb31alternate-emissive", "comb32alternate-emissive", "tied32-emissive", "crowd65_first-emissive"]
_NEE = {}


class Occupancy:
    """deep_trees.occupancy of model 0's tree (untransformed, opaque: culled) per ray, each distinct ray walked once"""

    def __init__(self, mesh):
        self.mesh, self.memo = mesh, {}

    def __call__(self, o, d):
        key = (np.asarray(o, dtype=F).tobytes(), np.asarray(d, dtype=F).tobytes())
        if key not in self.memo:
            self.memo[key] = dt.occupancy(self.mesh.nodes, o, d, self.mesh.tris, cull=True)[0]
        return self.memo[key]


def states_whose_first_sample_picks(orc, table, triangles, count, first=1 << 16):
    """The first `count` generator states from `first` on for which a path's first vertex, on an opaque surface, draws an entry of
    `triangles` from the light table: the draws in front of the sample's first are the specular draw and RandomDirection's
    (tests/nee_reference.py, Estimator.trace).  Only a choice of inputs: what the batch covers is asserted from the reference's logs."""
    found, o3 = [], F3()
    for s in range(first, first + (1 << 20)):
        st = C.c_uint32(s)
        orc.random_value(C.byref(st))
        orc.random_direction(C.byref(st), o3)
        if int(table["entries"][nr.pick(table["cdf"], F(orc.random_value(C.byref(st))))]["triangle"]) in triangles:
            found.append(s)
            if len(found) == count:
                break
    assert len(found) == count
    return np.array(found, dtype=np.int64)


def nee_arrays(pkg, api, name):
    """((meshInfo, triangles, nodes, spheres), RtParams) of a scene by name, as tests/radiance_reference.py::params_of makes them"""
    mgr = scene(pkg, name).make_manager(None, api, W, H)
    mgr.renderSeed = 5
    data = mgr.CreateAllMeshData(mgr.models)
    p = mgr.params()
    p.frame = FRAME
    return (data["meshInfo"], data["triangles"], data["nodes"], np.zeros(0, dtype=pkg.abi.sphere_dtype)), p


def nee_case(pkg, api, orc, name, estimator=nr.Estimator, accept=None, prefer=None, camera_states=None):
    """The scene's arrays and parameters, the witness state, witness_batch()'s pattern for this pass — 33 rays onto the catcher, the
    witness ray 64 times over, 33 camera rays onto the comb — and the reference's records and logs of that batch: computed once.
    `estimator`: the reference's class (tests/nee_reference.py's, or tests/mis_reference.py's: the draws in front of a path's first
    sample are the same).  `accept(probe, i)`: what else the probing run must say of ray i for its state to be the witness's;
    `prefer(probe, i)`: of the accepted states the first for which this holds too is taken, the first accepted one if there is none;
    `camera_states`: {k: state} for the k-th of the 33 camera rays in place of the state the frame gives it (a choice of inputs, like
    the witness's).  The defaults are the NEE case, byte for byte."""
    key = name if estimator is nr.Estimator else (name, estimator)
    if key in _NEE:
        return _NEE[key]
    abi = pkg.abi
    arrays, p = nee_arrays(pkg, api, name)
    height = height_of(name)
    mesh = scene(pkg, name).models[0].Mesh  # model 0: the tree, untransformed; its triangles are the uploaded triangles 0 ... H
    occ = Occupancy(mesh)
    tr = api.create_tracer(0)
    try:
        tr.upload_scene(*arrays)
        tr.set_params(p)
        # One run of the reference picks the generator states.  Rays 0 ... 63: the witness — a ray onto the catcher whose first vertex
        # samples a comb triangle with a shadow ray that fills the stack, and whose next segment fills it again — is the first of the
        # states 1 ... 64 for which the reference says so.  Behind them the 33 outer catcher rays, each with four candidate states whose
        # first sample falls on leaf 0.  The facing leaves hide one another and the far ones are the large ones, so in the deep combs a
        # shadow ray that reaches its triangle is rare (about one in 150), and in comb(1) only the blocker can stop one: an outer ray
        # takes the first of its candidates whose first shadow ray fills the stack and is unshadowed (even rays) or blocked (odd
        # rays), and keeps its own state if there is none.
        w_origin, w_dir = (CATCHER_POINT[0], CATCHER_POINT[1], 1.0), (0.0, 0.0, -1.0)
        k = np.arange(33)
        c_origins = np.stack([-0.24 + 0.015 * k, 0.2 - 0.0125 * k, np.ones(33)], axis=1)
        c_states = 1000 + 7919 * k
        table = nr.light_table(abi, arrays[0], arrays[1], arrays[3])
        candidates = states_whose_first_sample_picks(orc, table, {0}, 33 * 4).reshape(33, 4)
        probe = estimator(pkg, orc, tr, *[arrays[j] for j in (0, 1, 3)], p)
        probe.trace(abi.make_path_rays(np.concatenate([np.tile(w_origin, (64, 1)), np.repeat(c_origins, 4, axis=0)]), np.tile(w_dir, (64 + 132, 1)),
                                       np.concatenate([np.arange(1, 65), candidates.reshape(-1)])))
        first_shadow = {i: (o, d, obj, tri, seen) for (i, b, o, d, obj, tri, seen) in probe.shadow_log if b == 0}
        second_segment = {i: (o, d) for (i, b, o, d) in probe.segment_log if b == 1}
        state, preferred, tally = None, None, [sum(1 for i in first_shadow if i < 64), 0, 0]
        for i in range(64):
            if i not in first_shadow:
                continue
            o, d, obj, tri, _ = first_shadow[i]
            if not (obj == 0 and 0 <= tri <= height and occ(o, d) == height):
                continue
            tally[1] += 1
            if i in second_segment and occ(*second_segment[i]) == height and (accept is None or accept(probe, i)):
                tally[2] += 1
                state = i + 1 if state is None else state
                if prefer is not None and preferred is None and prefer(probe, i):
                    preferred = i + 1
        state = preferred if preferred is not None else state
        print(f"{name}: of the states 1 ... 64, {tally[0]} give the first vertex a shadow ray, {tally[1]} of those go to the comb with occupancy {height}, "
              f"{tally[2]} of those have a second segment of occupancy {height}; the witness state is {state}")
        assert state is not None, f"{name}: no witness among the states 1 ... 64: {tally}"
        for j in range(33):
            for m in range(4)[::-1]:
                i = 64 + 4 * j + m
                if i in first_shadow and first_shadow[i][4] == (j % 2 == 0) and occ(*first_shadow[i][:2]) == height:
                    c_states[j] = candidates[j, m]
        origins, dirs, states = rr.camera_rays(orc, p, W, H, FRAME)
        idx = np.arange(W * H)[2::11][:33]
        o = np.concatenate([c_origins, np.tile(w_origin, (64, 1)), origins.reshape(-1, 3)[idx]]).astype(F)
        d = np.concatenate([np.tile(w_dir, (33 + 64, 1)), dirs.reshape(-1, 3)[idx]]).astype(F)
        cam_states = states.reshape(-1)[idx].astype(np.int64)
        for k, v in (camera_states or {}).items():
            cam_states[k] = v
        s = np.concatenate([c_states, np.full(64, state), cam_states]).astype(np.uint32)
        rays = abi.make_path_rays(o, d, s)
        assert len(rays) == 130
        est = estimator(pkg, orc, tr, *[arrays[j] for j in (0, 1, 3)], p)
        want = est.trace(rays)
    finally:
        tr.close()
    for a in (rays, want):
        a.setflags(write=False)
    _NEE[key] = (arrays, p, height, occ, rays, want, est)
    return _NEE[key]


def assert_two_walk_coverage(name, height, occ, rays, est):
    """What the 130-ray batch covers, from the reference's logs (either estimator's: the logs have one shape): the 64 witness rays' first
    shadow rays and second segments stand on the last stack row, shadow rays there are blocked and let through, and some block has lanes
    with and without a shadow ray at vertex 0.  -> (full_shadows, full_segments, mixed)"""
    n = len(rays)
    shadow0 = {i: (o, d, seen) for (i, b, o, d, _, _, seen) in est.shadow_log if b == 0}
    full_shadows = [(i, b, seen) for (i, b, o, d, _, _, seen) in est.shadow_log if occ(o, d) == height]
    full_segments = [(i, b) for (i, b, o, d) in est.segment_log if occ(o, d) == height]
    # (every ray of a block starts in the same wave iteration, so vertex 0 of the 64 witness rays is one iteration in whichever wave holds them)
    assert all(i in shadow0 and occ(*shadow0[i][:2]) == height for i in range(33, 97)), "the 64 witness rays' first shadow rays"
    assert sum(1 for (i, b, _) in full_shadows if b == 0) >= 64
    assert any(seen for (_, _, seen) in full_shadows) and not all(seen for (_, _, seen) in full_shadows), "shadow rays on the last row: some unshadowed, some blocked"
    assert full_segments and any(b > 0 for (_, b) in full_segments), "a path segment on the last row"
    assert all(any(i == w and b == 1 for (i, b) in full_segments) for w in range(33, 97)), "the witness rays' second segments"
    mixed = []
    for first in range(0, n, 64):  # per block of 64 consecutive rays, the lanes of vertex 0 with and without a shadow ray
        lanes = range(first, min(first + 64, n))
        mixed.append((sum(1 for i in lanes if i in shadow0), len(lanes)))
    assert any(0 < with_shadow < lanes for (with_shadow, lanes) in mixed), mixed
    assert est.triangle_samples > 0 and est.shadow_rays > est.unshadowed > 0
    return full_shadows, full_segments, mixed


def assert_batch_in_every_order(name, tr, rays, want, host, buffers):
    """The batch through `host` (a tracer's host-form call) in order, reversed and as prefixes 1, 33, 96, 97 and 130, and through
    `buffers` (its device form) with 64 guard bytes of 0xa5 behind the records: the reference's records every time, the guard intact,
    and the 64 witness slots one and the same record.  -> the records in order"""
    n, guard = len(rays), 64
    got = host(rays)
    rev = host(rays[::-1])[::-1]
    prefixes = {k: host(rays[:k]) for k in (1, 33, 96, 97, 130)}
    d_rays, d_out = DevBuf(n * 32).upload(rays), DevBuf(n * 16 + guard, fill=0xa5)
    try:
        buffers(d_rays.ptr, n, d_out.ptr)
        tr.synchronize()
        raw = d_out.download(np.uint8)
    finally:
        d_rays.free(), d_out.free()
    for what, rec in [("in order", got), ("reversed", rev)] + [(f"n = {k}", part) for k, part in prefixes.items()]:
        ref = want[:len(rec)]
        bad = np.argwhere((rr.bits(rec["rgb"]) != rr.bits(ref["rgb"])).any(axis=1) | (rec["rng"] != ref["rng"])).ravel()
        assert not len(bad), f"{name}, {what}: {len(bad)} of {len(rec)} records differ; first is ray {bad[0]}: got {rec[bad[0]]}, want {ref[bad[0]]}"
        assert rec.tobytes() == ref.tobytes(), (name, what)
    assert raw[:n * 16].tobytes() == want.tobytes() and (raw[n * 16:] == 0xa5).all(), f"{name}: buffer form"
    assert len({r.tobytes() for r in got[33:97]}) == 1, "the 64 witness slots hold one and the same record"
    return got


@pytest.mark.parametrize("name", NEE_SCENES)
def test_nee_fills_the_last_stack_row_in_both_of_its_walks(pkg, api, orc, name):
    """rt_radiance_nee_kernel runs two run-to-completion walks per wave iteration through one LDS stack region: the path segments'
    (written out) and the shadow rays' (walk_all), with the feed's bookkeeping on the row behind the stack, extBase behind that, and
    lanes without a shadow ray parked while their neighbours push.  Here both walks stand on the last row, in the same iteration, for a
    whole wave's worth of lanes; everything bit for bit against tests/nee_reference.py, whose own walks (rt_query_closest) are tied to
    rt_debug_intersect on the same rays."""
    abi = pkg.abi
    t0 = time.perf_counter()
    arrays, p, height, occ, rays, want, est = nee_case(pkg, api, orc, name)
    t_ref = time.perf_counter() - t0
    assert p.maxBounceCount == 2 and np.isfinite(want["rgb"]).all() and want["rgb"].any()
    # ---- what the batch covers, from the reference's logs
    full_shadows, full_segments, mixed = assert_two_walk_coverage(name, height, occ, rays, est)
    table = nr.light_table(abi, arrays[0], arrays[1], arrays[3])
    assert table["n_triangle_entries"] >= height + 1 and table["n_sphere_entries"] == 0
    # ---- the device
    tr = api.create_tracer(0)
    try:
        tr.upload_scene(*arrays)
        tr.set_params(p)
        assert tr.nee_light_count() == (table["n_sphere_entries"], table["n_triangle_entries"])
        got = assert_batch_in_every_order(name, tr, rays, want, tr.radiance_trace_nee, tr.radiance_trace_nee_buffers)
        # the reference's own walks at this depth against the second device path
        seen_rays = {}
        for (_, _, o, d, _, _, _) in est.shadow_log:
            seen_rays.setdefault((o.tobytes(), d.tobytes()), (o, d))
        so, sd = np.array([v[0] for v in seen_rays.values()], dtype=F), np.array([v[1] for v in seen_rays.values()], dtype=F)
        hits, dbg = tr.query_closest(abi.make_rays(so, sd)), tr.debug_intersect(so, sd)
        if name == "comb32alternate-emissive":  # with the emitter put out the pass is rt_radiance_trace, bit for bit
            dark = arrays[0].copy()
            dark["material"]["emissionStrength"] = 0
            tr.update_models(dark)
            assert tr.nee_light_count() == (0, 0)
            plain, stripped = tr.radiance_trace(rays), tr.radiance_trace_nee(rays)
            assert stripped.tobytes() == plain.tobytes() and (stripped["rng"] != rays["rng"]).any() and stripped.tobytes() != got.tobytes()
    finally:
        tr.close()
    assert bits(dbg[:, 2]).tolist() == bits(hits["dst"]).tolist()
    assert bits(dbg[:, 3:6]).tolist() == bits(hits["normal"]).tolist() and bits(dbg[:, 6:9]).tolist() == bits(hits["pos"]).tolist()
    assert np.array_equal(dbg[:, 0] != 0, (hits["hit"] & 3) != 0) and np.array_equal(dbg[:, 1] != 0, (hits["hit"] & 0x100) != 0)
    print(f"{name}: {len(full_shadows)} shadow rays and {len(full_segments)} path segments with {height} stack entries; lanes of vertex 0 with a shadow ray per block {mixed}; "
          f"{len(so)} distinct shadow rays against rt_debug_intersect; reference {t_ref:.1f} s, all {time.perf_counter() - t0:.1f} s")


# ---------------------------------------------------------------- g. rt_mis: the bounce row and the reverse lookup behind the same two walks
def _mis_witness(probe, i):
    """ray i of the probing run: the hit that ends its second segment has its emission weighted by the balance heuristic with
    0 < wb < 1 — the lookup found an entry for the hit triangle, and both densities were computed"""
    return any(r == i and v == 1 and rule == mr.WEIGHTED and 0.0 < wb < 1.0 and kind == "triangle" for (r, v, wb, rule, kind) in probe.emission_log)


MIS_CAMERA_STATES = {"comb1alternate-emissive": {16: 77, 22: 81}}   # {scene: {k-th camera ray: generator state}}: see the test's text


def _mis_reaches_its_last_vertex(probe, i):
    """ray i of the probing run goes on to a diffuse vertex 2, where it must not sample"""
    return (i, 2) in probe.skipped_log


@pytest.mark.parametrize("name", NEE_SCENES)
def test_mis_fills_the_last_stack_row_in_both_of_its_walks(pkg, api, orc, name):
    """The MIS instantiations of rt_radiance_nee_kernel on the batch of (f) at maxBounceCount 2: vertices 0 and 1 sample, vertex 2 must
    not — the decision RT_SHADE_OPAQUE_END takes from the bounce count, which the > 64-model instantiation keeps in the LDS row behind
    the extension words, here (crowd65_first-emissive: one extension word) two rows behind a stack of 32 that both walks fill between
    the increment and the next read.  The witness's second segment ends on a comb triangle — a leaf at level H, named by
    hit_triangle() and looked up by rt_mis::entry_of — and its emission is weighted with 0 < wb < 1.  Everything bit for bit against
    tests/mis_reference.py; the witness rests on the geometric conditions tests/test_deep_trees.py holds for (f), no further one.
    Of the accepted states the witness prefers one whose path goes on to a skipped vertex 2.  comb(1) needs more: leaf 0 faces the
    camera and leaf 1 away from it, so a vertex on the comb or on the blocker sees no emitter's front, and only the 0.6 x 0.6 catcher
    can be a sampling vertex 1 or a diffuse vertex 2.  With the states the frame gives the camera rays no path of the batch gets there
    (0 rows in either log); MIS_CAMERA_STATES gives two of those rays a state, found by one search of 3,000 states per ray, whose path
    goes comb or blocker -> catcher (vertex 1: a sample that reaches its shadow walk) -> a diffuse vertex 2 (skipped)."""
    abi = pkg.abi
    t0 = time.perf_counter()
    arrays, p, height, occ, rays, want, est = nee_case(pkg, api, orc, name, mr.Estimator, _mis_witness, _mis_reaches_its_last_vertex, MIS_CAMERA_STATES.get(name))
    t_ref = time.perf_counter() - t0
    assert p.maxBounceCount == 2 and np.isfinite(want["rgb"]).all() and want["rgb"].any()
    # ---- what the batch covers, from the reference's logs
    full_shadows, full_segments, mixed = assert_two_walk_coverage(name, height, occ, rays, est)
    weights = {(r, v): (wb, rule, kind) for (r, v, wb, rule, kind) in est.emission_log}
    for w in range(33, 97):
        wb, rule, kind = weights[(w, 1)]
        assert rule == mr.WEIGHTED and 0.0 < wb < 1.0 and kind == "triangle", (w, wb, rule, kind)
    sampled = {v for (_, v, *_r) in est.sample_log}
    assert sampled == {0, 1}, f"vertices 0 and 1 sample, no other: {sampled}"
    assert est.skipped_log and all(v == 2 for (_, v) in est.skipped_log), "the last vertex takes no sample"
    mr.rules_allowed(est, name)
    models, triangles, spheres = arrays[0], arrays[1], arrays[3]
    objects, words, table = mr.map_arrays(abi, models, triangles, spheres)
    assert table["n_triangle_entries"] >= height + 1 and table["n_sphere_entries"] == 0
    got_map = api.light_map_arrays(models, triangles, spheres)
    assert got_map["objects"].tobytes() == objects.tobytes() and got_map["triangles"].tobytes() == words.tobytes(), f"{name}: rt_debug_light_map"
    assert got_map["n_entries"] == len(table["entries"]) and objects[0] == 0 and (words[:height + 1] != mr.NO_ENTRY).all(), "every leaf of the comb has an entry"
    # ---- the device
    second = next((o, d) for (i, b, o, d) in est.segment_log if i == 33 and b == 1)
    tr = api.create_tracer(0)
    try:
        tr.upload_scene(*arrays)
        tr.set_params(p)
        end = tr.query_closest(abi.make_rays(second[0][None], second[1][None]))[0]
        assert int(end["object"]) == 0 and 0 <= int(end["triangle"]) <= height, f"{name}: the witness's second segment ends on {end}"
        assert words[int(end["triangle"])] != mr.NO_ENTRY
        got = assert_batch_in_every_order(name, tr, rays, want, tr.radiance_trace_mis, tr.radiance_trace_mis_buffers)
        plain, nee = tr.radiance_trace(rays), tr.radiance_trace_nee(rays)
        assert got.tobytes() != plain.tobytes() and got.tobytes() != nee.tobytes(), "the batch tells the three estimators apart"
        if name == "comb32alternate-emissive":  # with the emitter put out the pass is rt_radiance_trace, bit for bit
            dark = arrays[0].copy()
            dark["material"]["emissionStrength"] = 0
            tr.update_models(dark)
            assert tr.nee_light_count() == (0, 0)
            plain, stripped = tr.radiance_trace(rays), tr.radiance_trace_mis(rays)
            assert stripped.tobytes() == plain.tobytes() and (stripped["rng"] != rays["rng"]).any() and stripped.tobytes() != got.tobytes()
    finally:
        tr.close()
    print(f"{name}: {len(full_shadows)} shadow rays and {len(full_segments)} path segments with {height} stack entries; lanes of vertex 0 with a shadow ray per block {mixed}; "
          f"the witness's second hit is triangle {int(end['triangle'])} with wb = {weights[(33, 1)][0]:.6f}; {len(est.sample_log)} shadow rays at vertices 0 and 1, "
          f"{len(est.skipped_log)} samples skipped at vertex 2; reference {t_ref:.1f} s, all {time.perf_counter() - t0:.1f} s")
