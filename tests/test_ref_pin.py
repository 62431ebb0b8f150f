"""The oracle pinned to the REFERENCE'S OWN TEXT (missing #1).

oracle/make_ref.py compiles /root/reference/Assets/Scripts/Tracer/RayCommon.hlsl + RayCompute.compute *as they stand*
(a listed set of syntactic rewrites, oracle/ref_compat.h for the HLSL types and intrinsics, include/rt_math.h for what
HLSL leaves to its compiler) into oracle/_ref/libref.so.  These tests demand that oracle/liboracle.so — the hand
restatement every other test in this repository compares the HIP kernels with — produces the SAME BITS as that library:
whole FrameRender / AccumulatedRender images of the BVH configs and of all five reference scenes, the shader's own
`stats` counters (RC:254,271), every intersection / shading / RNG function on random inputs, and the same again under the
RT_MATH_IEEE reading.  The reference has no sphere buffer (RC:341), so whole images of libref.so are model-only scenes and
RaySphere (RC:289-332) is compared at function level; the sphere extension's HOOK is pinned by libref_spheres.so = the same
text + the one declared semantic rewrite S1 of make_ref.py, on BASELINE configs 1 and 2 (round 5).

The rewrite list is checked to be syntactic: undoing each rewrite on the generated text gives back the reference's text
token for token (test_rewrites_are_only_the_listed_syntactic_ones).

Without the reference checkout (the GPU box) the prebuilt oracle/_ref/libref.so is used as it travels; without either
the tests skip.
"""
import ctypes as C
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

from bvh_support import mesh_cases
from fuzz_scenes import random_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

_spec = importlib.util.spec_from_file_location("rt_ref_lib", os.path.join(ROOT, "oracle", "ref_lib.py"))
ref_lib = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref_lib)

THREADS = min(16, os.cpu_count() or 8)


def _load_oracle(variant):
    spec = importlib.util.spec_from_file_location("rt_oracle_lib_" + (variant or "std"), os.path.join(ROOT, "oracle", "oracle_lib.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.load(graft.load_package(), variant=variant)


@pytest.fixture(scope="module")
def ref(pkg):
    lib = ref_lib.load(pkg)
    if lib is None:
        pytest.skip("oracle/_ref/libref.so absent and no reference checkout to build it from")
    return lib


def float32_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def render_pair(pkg, orc_lib, ref_lib_, scene_factory, w, h, frames, seed, tweak=None):
    """The same scene through the same RayComputeManager mirror on both libraries; the BVHs come from the oracle's
    builder either way (BVH.cs is C#, not part of the shader text)."""
    out = []
    for lib in (orc_lib, ref_lib_):
        tr = lib.create_tracer(THREADS)
        sc = scene_factory()
        sc.spheres = []
        mgr = sc.make_manager(tr, orc_lib, w, h)
        if tweak:
            tweak(mgr)
        mgr.OnEnable(renderSeed=seed)
        for _ in range(frames):
            mgr.RenderFrame()
        out.append((tr.read_accumulated(), tr.read_frame(), tr.counters(), tr.frame()))
        tr.close()
    return out


def assert_same(out, what):
    (acc_o, fr_o, c_o, f_o), (acc_r, fr_r, c_r, f_r) = out
    assert np.array_equal(float32_bits(fr_o), float32_bits(fr_r)), f"{what}: FrameRender differs in {int(np.any(float32_bits(fr_o) != float32_bits(fr_r), axis=-1).sum())} pixels"
    assert np.array_equal(float32_bits(acc_o), float32_bits(acc_r)), f"{what}: AccumulatedRender differs in {int(np.any(float32_bits(acc_o) != float32_bits(acc_r), axis=-1).sum())} pixels"
    assert f_o == f_r
    # the shader's own counters: stats[0] = triangle tests (RC:254), stats[1] = box tests = 2 per inner node (RC:271)
    assert c_o["triTests"] == c_r["triTests"] and c_o["innerSteps"] == c_r["innerSteps"], (what, c_o, c_r)
    assert c_o["segments"] == c_r["segments"] and c_o["pixelFrames"] == c_r["pixelFrames"]
    assert c_o["segments"] > 0


IMAGES = [  # (name, config, scene kwargs, width, height, frames, seed, manager tweak)
    ("config3", 3, {}, 96, 54, 3, 1, None),
    ("config3_sky_on", 3, {}, 64, 36, 2, 7, lambda m: setattr(m, "useSky", True)),
    ("config3_no_accumulate", 3, {}, 48, 27, 2, 3, lambda m: setattr(m, "accumulate", False)),
    ("config3_odd_size", 3, {}, 61, 35, 1, -5, None),
    ("config4_dof_subdiv3", 4, {"subdivisions": 3}, 80, 45, 2, 1, None),
    ("config4_dof_81920_triangles", 4, {"subdivisions": 6}, 64, 36, 1, 2, None),
    ("config5_class_4_meshes", 5, {"subdivisions": 4, "n_meshes": 4}, 64, 36, 1, 1, None),
    ("glass_balls.unity", 6, {}, 64, 36, 1, 1, None),
    ("glass_dragon.unity", 7, {}, 64, 36, 1, 1, None),
    ("sphere_refract.unity", 8, {}, 64, 36, 1, 1, None),
    ("splash.unity", 9, {}, 48, 27, 1, 1, None),
    ("text.unity", 10, {}, 64, 36, 1, 1, None),
]


@pytest.mark.parametrize("case", IMAGES, ids=[c[0] for c in IMAGES])
def test_oracle_equals_the_compiled_reference_text(pkg, orc, ref, case):
    name, cfg, kw, w, h, frames, seed, tweak = case
    out = render_pair(pkg, orc, ref, lambda: pkg.scenes.get(cfg, **kw), w, h, frames, seed, tweak)
    assert_same(out, name)


@pytest.mark.parametrize("seed", range(8))
def test_random_model_scenes(pkg, orc, ref, seed):
    """the fuzz generator of the GPU suite (random meshes, transforms with non-uniform scale, all three material flags,
    random camera / bounces / spp / sky / depth of field / BVH quality), spheres removed"""
    sc0, render_seed = random_scene(pkg, seed)
    if not sc0.models:
        pytest.skip("no models drawn for this seed")
    out = render_pair(pkg, orc, ref, lambda: random_scene(pkg, seed)[0], sc0.width, sc0.height, sc0.frames, render_seed)
    assert_same(out, f"fuzz {seed}")


def test_large_frame_index_and_seed_wrap(pkg, orc, ref):
    """quirk Q2: Frame * 719393 is an int32 multiply that wraps (RC:552)"""
    def tweak(m):
        m.numAccumulatedFrames = 0  # overwritten by OnEnable; the wrap is driven through set_params below
    out = []
    for lib in (orc, ref):
        tr = lib.create_tracer(THREADS)
        sc = pkg.scenes.get(3)
        mgr = sc.make_manager(tr, orc, 40, 24)
        mgr.OnEnable(renderSeed=2_000_000_000)
        mgr.numAccumulatedFrames = 5000  # 5000 * 719393 > 2^31
        mgr.RenderFrame()
        out.append((tr.read_accumulated(), tr.read_frame(), tr.counters(), tr.frame()))
        tr.close()
    assert_same(out, "frame 5000")


def test_the_other_reading_is_pinned_too(pkg):
    """liboracle_ieee.so == libref_ieee.so (-DRT_MATH_IEEE on both: IEEE '/', v / sqrt(dot), smoothstep with a divide)"""
    ref_i = ref_lib.load(pkg, variant="ieee")
    if ref_i is None:
        pytest.skip("oracle/_ref/libref_ieee.so absent and no reference checkout")
    orc_i = _load_oracle("ieee")
    for cfg, kw, w, h in ((3, {}, 64, 36), (4, {"subdivisions": 3}, 64, 36), (6, {}, 48, 27)):
        out = render_pair(pkg, orc_i, ref_i, lambda: pkg.scenes.get(cfg, **kw), w, h, 2, 1,
                          (lambda m: setattr(m, "useSky", True)) if cfg == 3 else None)
        assert_same(out, f"ieee config {cfg}")


# ------------------------------------------------------------------------------------------------ functions
def _f3(a):
    return np.ascontiguousarray(a, dtype=np.float32).ctypes.data_as(C.POINTER(C.c_float))


def _call(lib, name, n_out, *args):
    out = np.zeros(n_out, dtype=np.float32)
    getattr(lib, name)(*args, out.ctypes.data_as(C.POINTER(C.c_float)))
    return out


def _unit(rng):
    v = rng.normal(size=3)
    return (v / np.linalg.norm(v)).astype(np.float32)


def test_rng_functions(orc, ref):
    rng = np.random.default_rng(1)
    for s in [0, 1, 0xFFFFFFFF, 0x80000000] + [int(x) for x in rng.integers(0, 2**32, 2000)]:
        a, b = C.c_uint32(s), C.c_uint32(s)
        assert orc.next_random(C.byref(a)) == ref.next_random(C.byref(b)) and a.value == b.value
        assert float32_bits(orc.random_value(C.byref(a))) == float32_bits(ref.random_value(C.byref(b))) and a.value == b.value
        da = _call(orc, "random_direction", 3, C.byref(a))
        db = _call(ref, "random_direction", 3, C.byref(b))
        assert np.array_equal(float32_bits(da), float32_bits(db)) and a.value == b.value
        pa = _call(orc, "random_point_in_circle", 2, C.byref(a))
        pb = _call(ref, "random_point_in_circle", 2, C.byref(b))
        assert np.array_equal(float32_bits(pa), float32_bits(pb)) and a.value == b.value


def test_ray_triangle_box_sphere(pkg, orc, ref):
    rng = np.random.default_rng(2)
    tri = np.zeros(1, dtype=pkg.abi.triangle_dtype)
    for i in range(4000):
        pos = rng.uniform(-3, 3, 3).astype(np.float32)
        d = _unit(rng) * np.float32(rng.choice([1.0, 1.0, 0.3, 2.5]))  # local rays are not unit length (RC:352)
        if i % 7 == 0:
            d[rng.integers(0, 3)] = 0.0  # axis-parallel: invDir = inf (RC:221-226 relies on min/max NaN rules)
        for k in ("posA", "posB", "posC"):
            tri[0][k] = rng.uniform(-2, 2, 3)
        for k in ("normA", "normB", "normC"):
            tri[0][k] = _unit(rng)
        if i % 11 == 0:
            tri[0]["posC"] = tri[0]["posA"]  # degenerate: determinant 0
        for cull in (0, 1):
            a = _call(orc, "ray_triangle", 6, _f3(pos), _f3(d), tri.ctypes.data, cull)
            b = _call(ref, "ray_triangle", 6, _f3(pos), _f3(d), tri.ctypes.data, cull)
            assert np.array_equal(float32_bits(a), float32_bits(b)), (i, cull, a, b)
        lo = rng.uniform(-2, 1, 3).astype(np.float32)
        hi = (lo + rng.uniform(0, 2, 3)).astype(np.float32)
        if i % 5 == 0:
            pos = ((lo + hi) / 2).astype(np.float32)  # origin inside the box: dst 0
        if i % 13 == 0:
            pos[0] = lo[0]  # on a slab plane with a parallel ray: 0 * inf
        assert float32_bits(orc.ray_box(_f3(pos), _f3(d), _f3(lo), _f3(hi))) == float32_bits(ref.ray_box(_f3(pos), _f3(d), _f3(lo), _f3(hi)))
        centre = rng.uniform(-2, 2, 3).astype(np.float32)
        radius = float(rng.uniform(0.1, 2.5))
        a = _call(orc, "ray_sphere", 6, _f3(pos), _f3(d), _f3(centre), radius)
        b = _call(ref, "ray_sphere", 6, _f3(pos), _f3(d), _f3(centre), radius)
        assert np.array_equal(float32_bits(a), float32_bits(b)), (i, a, b)


def test_fresnel_refract_sky_material(pkg, orc, ref):
    rng = np.random.default_rng(3)
    mat = np.zeros(1, dtype=pkg.abi.material_dtype)
    for i in range(3000):
        n = _unit(rng)
        d = _unit(rng)
        ia, ib = (1.0, float(rng.uniform(1.0, 2.4))) if i % 2 else (float(rng.uniform(1.0, 2.4)), 1.0)
        assert float32_bits(orc.reflectance(_f3(d), _f3(n), ia, ib)) == float32_bits(ref.reflectance(_f3(d), _f3(n), ia, ib))
        assert np.array_equal(float32_bits(_call(orc, "refract", 3, _f3(d), _f3(n), ia, ib)), float32_bits(_call(ref, "refract", 3, _f3(d), _f3(n), ia, ib)))
        p = pkg.abi.RtParams()
        p.useSky = int(i % 9 != 0)
        p.sunFocus, p.sunIntensity = float(rng.uniform(50, 900)), float(rng.uniform(0, 20))
        p.sunColour[:] = [float(x) for x in rng.uniform(0, 1, 3)]
        p.dirToSun[:] = [float(x) for x in _unit(rng)]
        if i % 6 == 0:
            d[1] = np.float32(rng.uniform(-0.012, 0.002))  # around the ground / horizon smoothstep (RC:176)
        assert np.array_equal(float32_bits(_call(orc, "environment_light", 3, C.byref(p), _f3(d))),
                              float32_bits(_call(ref, "environment_light", 3, C.byref(p), _f3(d))))
        mat[0]["flag"] = int(rng.integers(0, 3))
        for k in ("diffuseCol", "emissionCol", "specularCol"):
            mat[0][k] = rng.uniform(0, 1, 4)
        pos = rng.uniform(-20, 20, 3).astype(np.float32)
        for spec in (0, 1):
            a = _call(orc, "material_colour", 3, mat.ctypes.data, _f3(pos), _f3(n), spec)
            b = _call(ref, "material_colour", 3, mat.ctypes.data, _f3(pos), _f3(n), spec)
            assert np.array_equal(float32_bits(a), float32_bits(b))


def test_ray_collision_and_single_pixels(pkg, orc, ref):
    rng = np.random.default_rng(4)
    trs = []
    for lib in (orc, ref):
        tr = lib.create_tracer(1)
        mgr = pkg.scenes.get(4, subdivisions=3).make_manager(tr, orc, 120, 68)
        mgr.OnEnable(renderSeed=9)
        trs.append(tr)
    for i in range(1500):
        pos = (rng.uniform(-2, 2, 3) + [0, 2, 0]).astype(np.float32)
        d = _unit(rng)
        a = _call(orc, "ray_collision", 10, trs[0].h, _f3(pos), _f3(d))
        b = _call(ref, "ray_collision", 10, trs[1].h, _f3(pos), _f3(d))
        if a[0] == 0 and b[0] == 0:
            continue  # a miss leaves the other fields undefined in the reference (RC:337)
        assert np.array_equal(float32_bits(a), float32_bits(b)), (i, a, b)
    for i in range(300):
        x, y, frame = int(rng.integers(0, 120)), int(rng.integers(0, 68)), int(rng.integers(1, 100))
        if i < 4:
            x, y = (119, 67) if i % 2 else (119, int(rng.integers(0, 68)))  # last column / row: quirk Q1
        a = _call(orc, "trace_pixel", 3, trs[0].h, x, y, frame)
        b = _call(ref, "trace_pixel", 3, trs[1].h, x, y, frame)
        assert np.array_equal(float32_bits(a), float32_bits(b)), (x, y, frame, a, b)
    for tr in trs:
        tr.close()


def test_spheres_are_refused_by_the_reference_text(pkg, orc, ref):
    tr = ref.create_tracer(1)
    mgr = pkg.scenes.get(1).make_manager(tr, orc, 16, 16)
    with pytest.raises(pkg.abi.RtError):
        mgr.OnEnable(renderSeed=1)
    tr.close()


# ------------------------------------------------------------------------------------------------ the sphere hook (S1)
@pytest.fixture(scope="module")
def ref_spheres(pkg):
    lib = ref_lib.load(pkg, "spheres")
    if lib is None:
        pytest.skip("oracle/_ref/libref_spheres.so absent and no reference checkout to build it from")
    return lib


def render_pair_with_spheres(pkg, orc_lib, ref_lib_, scene_factory, w, h, frames, seed, tweak=None):
    out = []
    for lib in (orc_lib, ref_lib_):
        tr = lib.create_tracer(THREADS)
        mgr = scene_factory().make_manager(tr, orc_lib, w, h)
        if tweak:
            tweak(mgr)
        mgr.OnEnable(renderSeed=seed)
        for _ in range(frames):
            mgr.RenderFrame()
        out.append((tr.read_accumulated(), tr.read_frame(), tr.counters(), tr.frame()))
        tr.close()
    return out


SPHERE_IMAGES = [  # BASELINE configs 1 and 2 — the headline image — and sphere + BVH mixtures
    ("config1_exact", 1, {}, 256, 256, 1, 1, None),
    ("config1_three_frames", 1, {}, 96, 96, 3, 5, None),
    ("config2_headline", 2, {}, 240, 135, 2, 1, None),
    ("config2_sky_off", 2, {}, 96, 54, 2, 3, lambda m: setattr(m, "useSky", False)),
    ("config2_dof", 2, {}, 96, 54, 1, 9, lambda m: (setattr(m, "defocusStrength", 60.0), setattr(m, "focusDistance", 7.0))),
]


@pytest.mark.parametrize("case", SPHERE_IMAGES, ids=[c[0] for c in SPHERE_IMAGES])
def test_oracle_equals_the_reference_text_with_the_sphere_hook(pkg, orc, ref_spheres, case):
    """libref_spheres.so = the reference's text + the declared rewrite S1 (make_ref.py): the reference's own RaySphere (RC:289-332)
    called from the place of its commented call (RC:341), the sphere's material in place of the hard-coded one.  The oracle's hook —
    order against the model loop, strict '<' between equal hits, the material substitution — must give the same bits, on BASELINE
    config 1 exactly and on config 2, the headline image."""
    name, cfg, kw, w, h, frames, seed, tweak = case
    out = render_pair_with_spheres(pkg, orc, ref_spheres, lambda: pkg.scenes.get(cfg, **kw), w, h, frames, seed, tweak)
    assert_same(out, name)


@pytest.mark.parametrize("seed", range(6))
def test_random_scenes_with_spheres_and_models(pkg, orc, ref_spheres, seed):
    """the GPU suite's fuzz generator WITH its spheres: spheres inside / in front of / behind meshes, glass spheres, equal hits"""
    sc0, render_seed = random_scene(pkg, seed)
    out = render_pair_with_spheres(pkg, orc, ref_spheres, lambda: random_scene(pkg, seed)[0], sc0.width, sc0.height, sc0.frames, render_seed)
    assert_same(out, f"fuzz {seed} with spheres")


def test_coincident_spheres_keep_the_first(pkg, orc, ref_spheres):
    """two identical spheres with different materials: strict '<' (the hook's `sphereHit.dst < result.dst`) keeps buffer order"""
    def factory():
        sc = pkg.scenes.get(1)
        import copy
        twin = copy.deepcopy(sc.spheres[0])
        twin.material.diffuseCol = (0.1, 0.9, 0.1, 1)
        sc.spheres.insert(1, twin)
        return sc
    out = render_pair_with_spheres(pkg, orc, ref_spheres, factory, 64, 64, 1, 1)
    assert_same(out, "coincident spheres")


def test_row_window_of_the_dispatcher(pkg, orc, ref_spheres):
    """ref_set_row_window (the dispatcher's, used by bench.py's in-run check at 1920x1080): strips of the reference text == the same
    strips of the oracle == those rows of the whole image"""
    W, H, strips = 96, 54, (0, 3, 6)
    imgs = []
    for lib in (orc, ref_spheres):
        whole = lib.create_tracer(THREADS)
        m = pkg.scenes.get(2).make_manager(whole, orc, W, H)
        m.OnEnable(renderSeed=1)
        m.RenderFrame()
        part = lib.create_tracer(THREADS)
        m2 = pkg.scenes.get(2).make_manager(part, orc, W, H)
        m2.OnEnable(renderSeed=1)
        for s_ in strips:
            m2.numAccumulatedFrames = 1
            m2.SetShaderParams()
            lib.set_row_window(part.h, s_ * 8, min(H, s_ * 8 + 8))
            part.render_frame()
        rows = np.concatenate([np.arange(s_ * 8, min(H, s_ * 8 + 8)) for s_ in strips])
        a, b = whole.read_accumulated(), part.read_accumulated()
        assert np.array_equal(float32_bits(a[rows]), float32_bits(b[rows]))
        other = np.setdiff1d(np.arange(H), rows)
        assert not b[other].any()
        imgs.append(b[rows])
        whole.close(), part.close()
    assert np.array_equal(float32_bits(imgs[0]), float32_bits(imgs[1]))


DEGENERATE = [(1, 1), (1, 13), (13, 1), (2, 2)]


@pytest.mark.parametrize("shape", DEGENERATE, ids=[f"{w}x{h}" for w, h in DEGENERATE])
def test_degenerate_images_equal_the_reference_text(pkg, orc, ref, ref_spheres, shape):
    """One pixel wide or high: uv = id.xy / (Resolution - 1) = 0 / 0 = NaN (RCC:15) for every pixel, so every primary ray has a NaN
    focus point and direction, and the float -> uint pixel coordinate (RC:551) converts NaN.  The oracle must give the reference
    text's bits and counters there too: config 2 (spheres, through the sphere hook) and config 3 (BVH models), 2 x 2 beside them."""
    w, h = shape
    for cfg, lib, pair in ((2, ref_spheres, render_pair_with_spheres), (3, ref, render_pair)):
        out = pair(pkg, orc, lib, lambda: pkg.scenes.get(cfg), w, h, 3, 4)
        assert_same(out, f"config {cfg} {w}x{h}")
        acc = out[1][0]
        assert np.all(np.isfinite(acc)) and np.all(acc[..., 3] == 3), f"config {cfg} {w}x{h}: the reference text's image"


@pytest.mark.skipif(not ref_lib.make_ref.available(), reason="needs the reference checkout")
def test_the_sphere_hook_is_the_only_semantic_rewrite():
    """Take S1's two insertions out of the --spheres translation unit: what is left is the plain translation unit, character for
    character — libref_spheres.so differs from libref.so by the declared hook and nothing else."""
    mk = ref_lib.make_ref
    plain, hooked = mk.translation_unit(), mk.translation_unit(spheres=True)
    assert plain != hooked
    with open(os.path.join(mk.SHADER_DIR, "RayCommon.hlsl"), encoding="utf-8-sig") as f:
        original = f.read().replace("\r\n", "\n")
    decl, hook, call = mk.rewrite(mk.S1_DECL), mk.rewrite(mk.S1_HOOK), mk.rewrite(mk.S1_COMMENTED_CALL)
    assert hooked.count(decl) == 1 and hooked.count(hook) == 1
    assert hooked.replace(decl, "").replace(hook, call) == plain
    # and the hook calls the reference's RaySphere, whose text is untouched (RC:289-332)
    a = original.index("ModelHitInfo RaySphere(")
    b = original.index("ModelHitInfo CalculateRayCollision(")
    assert mk.rewrite(original[a:b]) in hooked
    assert "RaySphere(worldRay.pos, worldRay.dir, sphere.centre, sphere.radius)" in hook


# ------------------------------------------------------------------------------------------------ stale libraries
def test_prebuilt_reference_libraries_match_the_committed_hashes():
    """oracle/_ref travels prebuilt to the GPU box, which cannot rebuild it: MANIFEST.json (written by every build) must name the
    inputs oracle/REF_EXPECTED.json names, the recipe files of this tree, and the libraries as they lie there."""
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libref.so")):
        pytest.skip("no prebuilt oracle/_ref")
    why = ref_lib.stale_reason(["libref.so", "libref_ieee.so", "libref_spheres.so", "libref_bvh.so"])
    assert why is None, why


@pytest.mark.skipif(not ref_lib.make_ref.available(), reason="needs the reference checkout")
def test_editing_the_recipe_without_rebuilding_is_noticed(tmp_path, monkeypatch):
    """the check reads the recipe files of the tree it runs in: a changed header with an unchanged library is stale"""
    mk = ref_lib.make_ref
    assert mk.check_manifest(["libref.so"]) is None
    real = mk._sha
    monkeypatch.setattr(mk, "_sha", lambda path: "0" * 64 if path.endswith("ref_compat.h") else real(path))
    why = mk.check_manifest(["libref.so"])
    assert why and "ref_compat.h" in why
    monkeypatch.setattr(mk, "_sha", lambda path: "0" * 64 if path.endswith("libref.so") else real(path))
    why = mk.check_manifest(["libref.so"])
    assert why and "libref.so" in why


# ------------------------------------------------------------------------------------------------ the recipe
@pytest.mark.skipif(not ref_lib.make_ref.available(), reason="needs the reference checkout")
def test_rewrites_are_only_the_listed_syntactic_ones():
    """Undo every rewrite of make_ref.rewrite() on its output: what is left must be the reference's text, token for token
    (apart from the dropped #pragma / #include / attribute / semantic tokens)."""
    mk = ref_lib.make_ref
    for name in mk.SOURCES:
        with open(os.path.join(mk.SHADER_DIR, name), encoding="utf-8-sig") as f:
            original = f.read().replace("\r\n", "\n")
        t = mk.rewrite(original)
        t = t.replace("int2 stats = {}; RefStatsExport stats_export(stats);", "int2 stats;")
        t = re.sub(r" = \{\};", ";", t)
        t = re.sub(r"\.(%s)\(\)" % "|".join(mk.SWIZZLES), r".\1", t)
        t = re.sub(r"\b(\w+)\{\}", r"(\1)0", t)
        t = re.sub(r"\b(\w+)& (\w+)", r"inout \1 \2", t)
        t = re.sub(r"\bhfloat\b", "float", t)
        t = re.sub(r"(\d)_h\b", r"\1", t)
        t = t.replace("HLSL_INF", "1.#INF")
        o = "\n".join(ln for ln in original.split("\n") if not re.match(r"\s*#\s*(pragma|include)\b", ln))
        o = re.sub(r"\[numthreads\([^)]*\)\]", "", o)
        o = re.sub(r"\s*:\s*SV_DispatchThreadID", "", o)
        o = re.sub(r"^const\s+(uint2|bool)\s+(\w+);", r"\1 \2;", o, flags=re.M)
        assert t.split() == o.split(), name


# ------------------------------------------------------------------------------------------------ BVH.cs
@pytest.fixture(scope="module")
def ref_bvh(pkg):
    lib = ref_lib.load_bvh(pkg)
    if lib is None:
        pytest.skip("oracle/_ref/libref_bvh.so absent and no reference checkout to build it from")
    return lib


def _bvh_meshes(pkg):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    return mesh_cases(pkg) + [pkg.meshes.icosphere(4, 1.0, 7), pkg.meshes.icosphere(5, 1.0, 2), pkg.meshes.rounded_cube(12)]


def _same_build(a, b):
    sa, sb = dict(a[2]), dict(b[2])
    sa.pop("timeMs"), sb.pop("timeMs")
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and sa == sb


@pytest.mark.parametrize("quality", [0, 1, 2])
def test_bvh_builders_equal_the_compiled_reference_bvh_text(pkg, api, orc, ref_bvh, quality):
    """BVH.cs:26-318 itself (oracle/make_ref.py --bvh: the C# text compiled as C++ after the listed syntactic rewrites) against the
    oracle's restatement and the product's host builder (one thread and five): nodes, triangle order and BuildStats byte for byte,
    on every mesh class incl. the degenerate ones (identical triangles, flat, point: NaN in CeilToInt)."""
    assert b"BVH.cs" in ref_bvh.version()
    for m in _bvh_meshes(pkg):
        r = ref_bvh.build_bvh_arrays(m.vertices, m.normals, m.triangles, quality)
        assert _same_build(orc.build_bvh_arrays(m.vertices, m.normals, m.triangles, quality), r), ("oracle", m.name)
        assert _same_build(api.build_bvh_arrays(m.vertices, m.normals, m.triangles, quality), r), ("product", m.name)
        for threads in (1, 5):
            assert _same_build(api.build_bvh_arrays_mt(m.vertices, m.normals, m.triangles, quality, threads), r), ("product mt", threads, m.name)


def test_bvh_benchmark_mesh_and_refusals_equal_the_reference_bvh_text(pkg, api, orc, ref_bvh):
    """The 81,920-triangle mesh of BASELINE configs 4 and 5; an empty mesh; and input whose split costs overflow (BVH.cs grows a chain of
    empty leaves there: all three refuse it with RT_ERR_SCENE instead of emitting a tree the shader cannot walk, RC:246)."""
    m = pkg.meshes.icosphere(6, 1.0, 4)
    assert m.triangle_count == 81920
    r = ref_bvh.build_bvh_arrays(m.vertices, m.normals, m.triangles, 1)
    assert _same_build(api.build_bvh_arrays(m.vertices, m.normals, m.triangles, 1), r)
    assert _same_build(orc.build_bvh_arrays(m.vertices, m.normals, m.triangles, 1), r)
    assert r[2]["leafNodeCount"] == (len(r[0]) + 1) // 2 and r[2]["triangleCount"] == 81920
    empty = (np.zeros((3, 3), np.float32), np.zeros((3, 3), np.float32), np.zeros(0, np.int32))
    assert _same_build(api.build_bvh_arrays(*empty, 1), ref_bvh.build_bvh_arrays(*empty, 1))
    assert _same_build(orc.build_bvh_arrays(*empty, 1), ref_bvh.build_bvh_arrays(*empty, 1))
    rng = np.random.default_rng(3)
    v = (rng.uniform(-1, 1, (64, 3)) * 3e19).astype(np.float32)      # extents ~1e20: area * count overflows to inf, inf < inf is false
    idx = rng.integers(0, 64, 3 * 40).astype(np.int32)
    outcomes = []
    for lib in (ref_bvh, orc, api):
        try:
            outcomes.append(("ok", lib.build_bvh_arrays(v, np.zeros_like(v), idx, 1)))
        except pkg.abi.RtError as e:
            outcomes.append(("refused", e.status))
    assert outcomes[0][0] == outcomes[1][0] == outcomes[2][0]
    if outcomes[0][0] == "ok":
        assert _same_build(outcomes[1][1], outcomes[0][1]) and _same_build(outcomes[2][1], outcomes[0][1])
    else:
        assert outcomes[0][1] == outcomes[1][1] == outcomes[2][1] == pkg.abi.RT_ERR_SCENE
    bad = idx.copy()
    bad[5] = 64
    for lib in (ref_bvh, orc, api):
        with pytest.raises(pkg.abi.RtError) as e:
            lib.build_bvh_arrays(v, np.zeros_like(v), bad, 1)
        assert e.value.status == pkg.abi.RT_ERR_INVALID_ARG


@pytest.mark.skipif(not ref_lib.make_ref.bvh_available(), reason="needs the reference checkout")
def test_bvh_rewrites_are_only_the_listed_syntactic_ones():
    """Undo the rewrites of make_ref.rewrite_bvh() on its output and compare with BVH.cs line by line (as a multiset: B3 moves the
    nested types in front of their first use).  What is not undone is applied to the original instead and is named here: the cut
    members (B2), the dropped modifiers (B4), `class` -> `struct`, and the switch expressions (B12)."""
    mk = ref_lib.make_ref
    with open(mk.BVH_SOURCE, encoding="utf-8-sig") as f:
        original = f.read().replace("\r\n", "\n").replace("\t", "    ")
    t = mk.rewrite_bvh(original)
    t = re.sub(r"^\s*\w+\(\) = default;\n", "", t, flags=re.M)                                       # B18
    t = t.replace("Quality Quality_;", "Quality Quality;").replace("this->Quality_ = quality;", "this->Quality = quality;")   # B17
    t = re.sub(r"^(\s*)(int|float) (\w+)\{\};", r"\1\2 \3;", t, flags=re.M)                            # B16
    t = t.replace("int NodeCount() const { return Index; }", "int NodeCount => Index;").replace(".NodeCount()", ".NodeCount")   # B15
    t = t.replace("this->", "this.")                                                                 # B14
    t = t.replace("Array::Resize(", "Array.Resize(ref ")                                             # B13
    t = re.sub(r"\b(Mathf|Math|Quality)::", r"\1.", t)
    t = re.sub(r"return std::make_tuple\(([^;]*)\);", r"return (\1);", t)                            # B11
    t = t.replace("std::tuple<int, float, float> ", "(int axis, float pos, float cost) ")
    t = re.sub(r"auto \[(\w+), (\w+), (\w+)\] = ", r"(int \1, float \2, float \3) = ", t)
    t = re.sub(r"(?<![\w.])(\d+)\.0f\b", r"\1f", t)                                                   # B10
    for cs, cpp in (("float.MaxValue", "CS_FLOAT_MAX"), ("float.MinValue", "CS_FLOAT_MIN"),          # B9
                    ("float.PositiveInfinity", "CS_FLOAT_POSITIVE_INFINITY"), ("int.MaxValue", "CS_INT_MAX")):
        t = t.replace(cpp, cs)
    t = re.sub(r"\bauto\b", "var", t)                                                                # B8
    t = t.replace("Stopwatch::StartNew()", "System.Diagnostics.Stopwatch.StartNew()")
    t = re.sub(r"\b(\w+)& (\w+) = ", r"ref \1 \2 = ref ", t)                                          # B7
    t = re.sub(r"= \{\};", "= new();", t)                                                            # B6
    t = re.sub(r"\b(\w+) (\w+) = \1\(", r"\1 \2 = new(", t)
    t = re.sub(r"CsArray<(\w+)>\(([^)]+)\)", r"new \1[\2]", t)                                        # B5
    t = re.sub(r"CsArray<(\w+)>", r"\1[]", t)
    t = re.sub(r"\benum class\b", "enum", t)                                                         # B4
    t = re.sub(r"\}\s*;", "}", t)                                                                    # B3
    t = re.sub(r"namespace (\w+)::(\w+)", r"namespace \1.\2", t)                                      # B1

    o = "\n".join(ln for ln in original.split("\n") if not re.match(r"\s*using\s+[\w.]+;", ln)).replace("[System.Serializable]", "")
    for pat in mk.BVH_CUT:
        a, b = mk._block(o, pat)
        o = o[:a] + o[b:]
    o = re.sub(r"\n\s*// ---- Traversal ---\s*\n", "\n", o)
    o = re.sub(r"\b(public|readonly|private|override)\s+", "", o)
    o = re.sub(r"\bclass\b", "struct", o)
    o = re.sub(r"(\w+) switch\s*\{\s*0 => ([^,]+),\s*1 => ([^,]+),\s*_ => ([^}]+?)\s*\};", r"(\1 == 0 ? \2 : \1 == 1 ? \3 : \4);", o)
    o = re.sub(r"\bnew (\w+)\(", r"\1(", o)            # `new T(args)` -> `T(args)` (B6) cannot be told from a call afterwards: applied here
    o = re.sub(r"\}\s*;", "}", o)

    def lines(s):
        return sorted(" ".join(ln.split()) for ln in s.split("\n") if ln.strip())
    assert lines(t) == lines(o)
