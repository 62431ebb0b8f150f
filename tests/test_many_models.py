"""The catalogue of tests/many_models.py on the CPU: the conditions tests/test_gpu_many_models.py rests on.

  1. the scenes are what the catalogue says (sizes, model counts, the filtered range, tree height, FLAT or not), and rt_scene_prep.h
     never filters the models planted as unfilterable;
  2. the oracle equals the reference text (oracle/_ref/libref.so) on every scene: both images after one frame and after two more,
     segments, triangle tests and inner steps.  tests/test_hazards.py's rules: a stale library fails, an absent one skips;
  3. on the staircase every index of WITNESS is the first hit of some pixel-centre ray, in both orders;
  4. a float64 slab test shows that the ray of pixel W_PIXEL meets the world box of ALL models of the staircase;
  5. no expected image holds a NaN pixel;
  6. rt_launch_plan.h gives a 32-level tree beside 1,300 models the largest wave region there is: one group of 9 waves around a
     24-record cache, 162,816 B of LDS (tests/launch_plan_driver.cpp);
  7. the order in which a lane visits its candidates and the unfiltered tail, replayed on the host around the helper the kernel uses
     (tests/many_tail_driver.cpp), plainly and under the address and undefined-behaviour sanitizers, as a stand-alone program."""
import os
import subprocess
import sys

import numpy as np
import pytest

import host_driver
import many_models as mm
import scene_prep_support as sp
from launch_plan_support import one, plan  # noqa: F401  (plan: the fixture that builds tests/launch_plan_driver.cpp)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

ref_lib = graft._ref_lib()


# ---- 1. the catalogue ----------------------------------------------------------------------------------------------------------------

def _count(name):
    digits = "".join(c for c in name if c.isdigit())
    return mm.N_STAIRS if name.startswith("stairs-") else int(digits) + (1 if name.startswith("comb_") else 0)


@pytest.mark.parametrize("name", mm.CATALOGUE)
def test_scene_is_what_the_catalogue_says(pkg, api, orc, name):
    sc = mm.scene(pkg, orc, name)
    assert sc.w <= 48 and sc.h <= 32 and sc.p.numRaysPerPixel == 2 and sc.p.useSky == 1 and len(sc.spheres) == 0
    assert sc.n == _count(name) > 64
    v = api.validate_scene_arrays(sc.models, sc.triangles, sc.nodes, sc.spheres)
    assert v["flat"] == (1 if name.startswith("flat") else 0)
    assert v["n_filtered"] == min(sc.n, mm.FILTER_CAP)
    if name in mm.COMB_SCENES:
        assert v["max_height"] == 32
        comb = 0 if "first" in name else sc.n - 1
        assert sc.tri_count[comb] == 33 and (comb >= mm.FILTER_CAP) == (name == "comb_last1299")
    else:
        assert v["max_height"] < 30


def test_edges_are_the_ends_of_the_mask():
    """the counts of N_EDGES against the layout of the candidate set: models 63 ... 94 are word 0, 95 ... 126 word 1, 1055 ... 1086 word 31"""
    word = lambda m: (m - 63) >> 5   # noqa: E731
    assert word(94 - 1) == 0 and (94 - 1 - 63) & 31 == 30 and word(95 - 1) == 0 and (95 - 1 - 63) & 31 == 31   # 95 models: bit 31 of word 0
    assert word(96 - 1) == 1 and (96 - 1 - 63) & 31 == 0 and word(127 - 1) == 1 and (127 - 1 - 63) & 31 == 31
    assert word(1087 - 1) == 31 and (1087 - 1 - 63) & 31 == 31 and word(1086 - 1) == 31 and (1086 - 1 - 63) & 31 == 30
    assert mm.FILTER_CAP == 63 + 32 * 32 and set(mm.N_EDGES) >= {mm.FILTER_CAP - 1, mm.FILTER_CAP, mm.FILTER_CAP + 1, mm.FILTER_CAP + 2}
    for w in mm.WITNESS + mm.ALWAYS + mm.EMITTERS:
        assert 0 <= w < mm.N_STAIRS
    assert {i for i in mm.WITNESS if i >= mm.FILTER_CAP} == {1087, 1088, 1299} and {i for i in mm.ALWAYS if i >= mm.FILTER_CAP} == {1087, 1299}


def test_planted_models_are_never_filtered(pkg, orc, tmp_path):
    """always1300 through rt_scene_prep.h (tests/scene_prep_driver.cpp): the filter records of the planted models say `always`, the
    unusable leaf root with count 0, and those of crowd1300 at the same indices do not"""
    exe = host_driver.build(tmp_path, "scene_prep", ["-std=c++17", "-O2"], after=["-pthread"])
    always = {}
    for name in ("always1300", "crowd1300"):
        sc = mm.scene(pkg, orc, name)
        path = str(tmp_path / f"{name}.scene")
        sp.write_scene(path, sc.models, sc.triangles, sc.nodes, sc.spheres)
        info, raw = sp.ask(exe, [f"load {path}", "validate", "dump filters"])[1:]
        assert info["rc"] == 0 and info["flat"] == 0 and info["n_filtered"] == mm.FILTER_CAP, info
        f = np.frombuffer(raw, dtype=sp.FILTER)
        assert len(f) >= mm.FILTER_CAP
        always[name] = f
    planted = [i for i in mm.ALWAYS if i < mm.FILTER_CAP]
    assert planted == [62, 63, 1086]
    for i in planted:
        assert always["always1300"][i]["always"] == 1 and always["crowd1300"][i]["always"] == 0, i
    assert always["always1300"][mm.ALWAYS_LEAF]["innerRoot"] == 0
    assert all(always["always1300"][i]["innerRoot"] == 1 for i in planted if i != mm.ALWAYS_LEAF)


# ---- 2. the oracle against the reference text --------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ref(pkg):
    lib = ref_lib.load(pkg, "")
    if lib is None:
        return None
    why = ref_lib.stale_reason(["libref.so"])
    if why:
        pytest.fail("stale reference library: " + why)
    return lib


@pytest.mark.parametrize("name", mm.CATALOGUE)
def test_the_oracle_equals_the_reference_text(pkg, orc, ref, name):
    if ref is None:
        pytest.skip("oracle/_ref is not here (built from the reference checkout)")
    tr = ref.create_tracer(8)
    try:
        if name in mm.COMB_SCENES:
            # the reference's driver (oracle/ref_driver.h) lets at most 31 levels, the root counted, reach the text's int stack[32]
            with pytest.raises(pkg.abi.RtError) as e:
                mm.drive(mm.scene(pkg, orc, name), tr)
            assert "int stack[32]" in str(e.value), str(e.value)
            return
        got = mm.drive(mm.scene(pkg, orc, name), tr)
    finally:
        tr.close()
    want = mm.expected(pkg, orc, name)
    for part, g, o in (("one frame", got[0], want[0]), ("then 2 fused frames", got[1], want[1])):
        assert np.array_equal(o[0].view(np.uint32), g[0].view(np.uint32)), f"{name}, {part}: the oracle's AccumulatedRender != the reference text's"
        assert np.array_equal(o[1].view(np.uint32), g[1].view(np.uint32)), f"{name}, {part}: the oracle's FrameRender != the reference text's"
    for k in ("segments", "triTests", "innerSteps", "pixelFrames"):
        assert got[2][k] == want[2][k], (name, k, got[2][k], want[2][k])


# ---- 3, 4. the witness conditions ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["near_first", "near_last"])
def test_every_witness_plate_is_the_first_hit_of_a_pixel(pkg, orc, order):
    sc = mm.scene(pkg, orc, f"stairs-{order}")
    first = mm.first_hit_models(pkg, orc, sc)
    seen = {int(i): int((first == i).sum()) for i in np.unique(first)}
    print(f"stairs-{order}: pixels per first-hit model {seen}")
    for w in mm.WITNESS:
        assert seen.get(w, 0) >= 4, (order, w, seen)
    assert set(seen) - {-1} == set(mm.WITNESS)   # a plate that is no witness is hidden behind one that is
    assert first[mm.W_PIXEL[1], mm.W_PIXEL[0]] == (0 if order == "near_first" else sc.n - 1)


@pytest.mark.parametrize("order", ["near_first", "near_last"])
def test_one_ray_meets_the_world_box_of_every_model(pkg, orc, order):
    """float64: the hull of the mesh's root box through each model's localToWorld, and the slab test of W_PIXEL's pixel-centre ray against
    it.  The filter's boxes are inflated supersets of these world boxes (tests/test_scene_prep.py::test_root_filter_boxes: they hold
    the float64 hull of the root's children, which fill the root's box here), and nothing is hit when the filter runs: a ray that meets
    a model's world box KEEPS that model as a candidate, so this lane has all 1,300 — every summary bit and every bit of every word."""
    sc = mm.scene(pkg, orc, f"stairs-{order}")
    origins, dirs = mm.pixel_centre_rays(sc)
    o, d = origins[mm.W_PIXEL[1], mm.W_PIXEL[0]].astype(np.float64), dirs[mm.W_PIXEL[1], mm.W_PIXEL[0]].astype(np.float64)
    assert len({int(m["nodeOffset"]) for m in sc.models}) == 1
    root = sc.nodes[int(sc.models[0]["nodeOffset"])]
    assert root["triangleCount"] <= 0, "the plates' mesh has an inner root"
    lo, hi = root["boundsMin"].astype(np.float64), root["boundsMax"].astype(np.float64)
    corners = np.array([[(hi if c >> k & 1 else lo)[k] for k in range(3)] for c in range(8)])
    shortest = np.inf
    for i in range(sc.n):
        m = sc.models[i]["localToWorld"].astype(np.float64).reshape(4, 4).T
        pts = corners @ m[:3, :3].T + m[:3, 3]
        with np.errstate(divide="ignore"):
            t0, t1 = (pts.min(0) - o) / d, (pts.max(0) - o) / d
        near, far = np.minimum(t0, t1).max(), np.maximum(t0, t1).min()
        assert far > max(near, 0.0), (order, i, near, far)
        shortest = min(shortest, far - max(near, 0.0))
    assert shortest > 1e-3   # a segment, far above fp32's resolution at these depths (1e-6)
    print(f"stairs-{order}: the ray of pixel {mm.W_PIXEL} is inside every one of {sc.n} world boxes for at least {shortest:.4f}")


# ---- 5. no NaN pixels --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", mm.CATALOGUE)
def test_no_expected_image_holds_a_nan(pkg, orc, name):
    single, fused, c = mm.expected(pkg, orc, name)
    sc = mm.scene(pkg, orc, name)
    for img in single + fused:
        assert np.isfinite(img).all(), name
        assert img[..., :3].any(), name
    assert c["pixelFrames"] == 3 * sc.w * sc.h and c["modelVisits"] == c["segments"] * sc.n and c["sphereTests"] == 0
    assert (c["innerSteps"] == 0) == name.startswith("flat")


# ---- 6. the LDS plan ---------------------------------------------------------------------------------------------------------------------

def test_lds_plan_of_a_32_level_tree_beside_1300_models(plan):  # noqa: F811
    """a wave's region is (32 stack rows + 4 pixel fields + 2 + 32 extension rows) x 256 B = 17,920 B; 9 of them fit a CU's 160 KB, so
    one group of 9 waves, and the 1,536 B its share leaves (less the 1 KB kept clear) make a 24-record cache: 162,816 B, 1 KB under the CU's"""
    waves, records, lds = mm.EXTREME_GROUP
    for models in (1087, 1088, 1300):   # (every count from 1,056 on has 32 extension words)
        f = one(plan, "filter", models=models)
        assert f == {"nf": mm.FILTER_CAP, "ext": 32}
        assert one(plan, "groups", height=32, models=models, want=12) == {"wpg": waves, "records": records}
    assert (waves, records) == (9, 24)
    for stats in (0, 1):
        s = one(plan, "shape", flat=0, stats=stats, stack=32, ext=32, chunks=82, hot=4 * records, wpg=waves, cus=256, tiles=6, frames=1)
        assert s["lds"] == lds == 162816 and s["lds"] <= 160 * 1024 and s["threads"] == 64 * waves and s["wavedwords"] == 70 * 64
        assert s["many"] == 1 and s["hot"] == 1 and s["variant"] == 10 + stats
    # without the cache (RT_HOT_KB=0): single waves of 17,920 B, variants 4 and 5
    assert one(plan, "groups", height=32, models=1300, want=12, hotkb=0) == {"wpg": 1, "records": 0}
    s = one(plan, "shape", flat=0, stats=0, stack=32, ext=32, chunks=82, hot=0, wpg=1, cus=256, tiles=6, frames=1)
    assert (s["lds"], s["threads"], s["variant"]) == (17920, 64, 4)


# ---- 7. the tail rule, on the host ---------------------------------------------------------------------------------------------------------

def test_tail_rule_visits_every_model_once_in_order(tmp_path):
    """tests/many_tail_driver.cpp around rt_plan::next_unfiltered_model, the expression rt_kernels.h's vote and phase A share: n = 65,
    1087, 1088 and 1300 models; no candidate, all, only 1086, all but 1086, every word alone, the ends of every word, 200 random sets.
    Built plainly (warning-free) and with the sanitizers linked into the program; nothing sanitized is loaded into python."""
    plain = host_driver.build(tmp_path, "many_tail", ["-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror"], exe="tail")
    san = host_driver.build(tmp_path, "many_tail", ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"],
                            exe="tail_san")
    for exe in (plain, san):
        p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and p.stdout.strip() == "MANY_TAIL_OK", (exe, p.returncode, p.stdout[-300:], p.stderr[-3000:])


def test_kernel_and_driver_share_the_tail_rule():
    """the helper is what the kernel calls, in the vote and in phase A, and the expression stands nowhere else in it"""
    kernels = open(os.path.join(ROOT, "ray-tracing_amd", "csrc", "rt_kernels.h")).read()
    assert kernels.count("rt_plan::next_unfiltered_model(t.m, a.nFiltered)") == 2
    assert "a.nFiltered - 1" not in kernels
    plan_h = open(os.path.join(ROOT, "ray-tracing_amd", "csrc", "rt_launch_plan.h")).read()
    assert "RT_HD int next_unfiltered_model(int m, int nFiltered) { return m < nFiltered - 1 ? nFiltered : m + 1; }" in plan_h
