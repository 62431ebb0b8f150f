"""The family of in-cap scenes of tests/capfuzz_scenes.py through the two host drivers, and the conditions on the family itself (no GPU).

Every seed's scene, as the part of the image its seed renders, is written in the text forms of tests/tile_cand_driver.cpp and
tests/tile_tri_driver.cpp and run through their sanitizer builds (stand-alone executables with the runtimes linked in, as in
tests/test_tile_cand.py) over every tile: no sphere and no triangle that accepts a camera ray may be missing from its tile's mask.

tests/test_gpu_tile_fuzz.py renders the same scenes on the device; what it can find depends on what the family reaches, so that is
asserted here, on the CPU, where the scenes are the same bits as there (the generator draws from meshes._lcg):
  - among the scenes with a sphere, at least half have a tile whose sphere mask is not all ones (mean_mask < the sphere count);
  - among the scenes with a triangle, at least half have a tile whose triangle mask is not all ones;
  - at least a quarter of the scenes with a triangle have a tile with an EMPTY triangle mask (share0 > 0): the tw.wave == 0 skip of
    traverse_flat; and each of capfuzz_scenes.EMPTY_TRI_MASK_SEEDS, which the GPU half measures the saved work on, is one of them;
  - no oracle image of the family holds a NaN (a NaN has no agreed bit pattern to compare);
  - every listed sphere count, triangle split, field of view, diverge strength and bounce count occurs, a third of the scenes have the
    camera inside or next to a sphere, a quarter are parts of strip partitions;
  - every scene is within every cap, and every scene of scene_over_a_cap is over exactly the one it names."""
import os
import re
import subprocess

import numpy as np
import pytest

import capfuzz_scenes as cs
import host_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_SPHERES, MAX_MODELS, MAX_TRIS = 32, 4, 16   # RT_PRIMARY_MAX_* of ray-tracing_amd/csrc/rt_primary.h


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("tile_fuzz")
    out = {"dir": d}
    for name in ("tile_cand", "tile_tri"):
        out[name] = host_driver.build(d, name, ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                "-static-libasan", "-static-libubsan"], exe=name + "_san")
    return out


def _run(exe, path):
    """`scene FILE 1`: every tile.  -> (why it failed or None, the figures of the last line)"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("RT_")}
    p = subprocess.run([exe, "scene", path, "1"], capture_output=True, env=env, timeout=600)
    out = p.stdout.decode(errors="replace")
    last = (out.strip().splitlines() or [""])[-1]
    ok = p.returncode == 0 and last.startswith("ok ") and " misses=0 " in last + " "
    return (None if ok else (p.returncode, out[-3000:], p.stderr.decode(errors="replace")[-3000:])), {k: float(v) for k, v in re.findall(r"(\w+)=([-0-9.e+]+)", last)}


def _root_leaf_counts(api, sc):
    """triangles in every model's root, 0 for a root that is not a leaf"""
    mgr = sc.make_manager(cs._NoTracer(), api)
    data = mgr.CreateAllMeshData(mgr.models)
    return [max(int(data["nodes"][int(m["nodeOffset"])]["triangleCount"]), 0) for m in data["meshInfo"]]


def _over(api, sc):
    """the caps a scene exceeds"""
    leaves = _root_leaf_counts(api, sc)
    over = []
    if len(sc.spheres) > MAX_SPHERES:
        over.append("33 spheres")
    if len(sc.models) > MAX_MODELS:
        over.append("5 models")
    if all(leaves) and sum(leaves) > MAX_TRIS:
        over.append("17 triangles")
    if sc.settings["defocusStrength"] != 0.0:
        over.append("defocusStrength = 1e-30")
    if not all(leaves):
        over.append("a root that is not a leaf")
    return over


@pytest.fixture(scope="module")
def family(pkg, api, orc, drivers):
    """per seed: the scene, the two drivers' outcomes on its part of the image and whether the oracle's image (1 + 2 frames) is finite"""
    out = {}
    for seed in cs.SEEDS:
        sc, render_seed = cs.scene(pkg, seed)
        part = cs.partition_of(seed) or (8, 0, 1)
        rec = {"scene": sc, "part": part}
        rec["sph_fail"], rec["sph"] = _run(drivers["tile_cand"], cs.write_sphere_scene(pkg, api, sc, str(drivers["dir"] / f"s{seed}.txt"), part=part))
        rec["tri_fail"], rec["tri"] = _run(drivers["tile_tri"], cs.write_triangle_scene(pkg, api, sc, str(drivers["dir"] / f"t{seed}.txt"), part=part))
        tr = orc.create_tracer(8)
        mgr = sc.make_manager(tr, orc)
        mgr.OnEnable(renderSeed=render_seed)
        mgr.RenderFrame()
        mgr.RenderFrames(2)
        rec["finite"] = bool(np.isfinite(tr.read_accumulated()).all() and np.isfinite(tr.read_frame()).all())
        tr.close()
        out[seed] = rec
        print(f"seed {seed}: {sc.width}x{sc.height} part {part} fov {sc.camera.fieldOfView} spheres {len(sc.spheres)} triangles {cs.triangle_counts(sc)} "
              f"bounces {sc.settings['maxBounceCount']} diverge {sc.settings['divergeStrength']}: sphere mean_mask {rec['sph'].get('mean_mask')} "
              f"triangle mean_mask {rec['tri'].get('mean_mask')} share0 {rec['tri'].get('share0')} finite {rec['finite']}")
    return out


def test_the_family_is_as_large_as_it_says():
    assert 24 <= len(cs.SEEDS) <= 32 and len(set(cs.SEEDS)) == len(cs.SEEDS)


@pytest.mark.parametrize("seed", cs.SEEDS)
def test_no_accepted_sphere_or_triangle_is_missing_from_a_tile_mask(family, seed):
    rec = family[seed]
    assert rec["sph_fail"] is None, rec["sph_fail"]
    assert rec["tri_fail"] is None, rec["tri_fail"]
    assert rec["sph"]["spheres"] == len(rec["scene"].spheres) and rec["tri"]["triangles"] == sum(cs.triangle_counts(rec["scene"]))
    assert rec["sph"]["checked"] == rec["sph"]["tiles"] > 0 and rec["tri"]["checked"] == rec["tri"]["tiles"] > 0   # stride 1: every tile


@pytest.mark.parametrize("seed", cs.SEEDS)
def test_every_scene_is_within_every_cap(pkg, api, seed):
    sc, _ = cs.scene(pkg, seed)
    assert _over(api, sc) == []
    assert sc.settings["bvhQuality"] == pkg.abi.BVH_QUALITY_DISABLED and sc.settings["defocusStrength"] == 0.0
    assert 9 <= sc.width <= 80 and 9 <= sc.height <= 50
    mgr = sc.make_manager(cs._NoTracer(), api)
    values = [*mgr.params().camLocalToWorld, *mgr.params().viewParams]
    for s in sc.spheres:
        assert 0.02 <= s.radius <= 3.0
        values += [*s.centre, s.radius]
    for m in mgr.CreateAllMeshData(mgr.models)["meshInfo"]:
        values += [*m["worldToLocal"], *m["localToWorld"]]
    for m in sc.models:
        values += list(m.Mesh.vertices.reshape(-1))
    assert np.isfinite(np.array(values, dtype=np.float32)).all()


@pytest.mark.parametrize("seed", range(10))
def test_every_over_a_cap_scene_is_over_exactly_the_cap_it_names(pkg, api, seed):
    sc, _ = cs.scene_over_a_cap(pkg, seed)
    over = _over(api, sc)
    kind = cs.OVER_A_CAP_KINDS[seed % 5]
    if kind == "a root that is not a leaf":
        assert over == [kind] and len(sc.models) <= MAX_MODELS and max(cs.triangle_counts(sc)) > MAX_TRIS
    else:
        assert over == [kind]
    if kind == "33 spheres":
        assert len(sc.spheres) == 33
    if kind == "5 models":
        assert len(sc.models) == 5
    if kind == "17 triangles":
        assert sum(cs.triangle_counts(sc)) == 17
    if kind == "defocusStrength = 1e-30":
        assert np.float32(sc.settings["defocusStrength"]) == np.float32(1e-30) != 0
    # nothing else moved: the camera and the settings are the in-cap scene's
    base, _ = cs.scene(pkg, seed)
    assert (base.width, base.height, base.camera.fieldOfView, base.camera.transform.position, base.camera.transform.euler) == \
           (sc.width, sc.height, sc.camera.fieldOfView, sc.camera.transform.position, sc.camera.transform.euler)
    assert {k: v for k, v in base.settings.items() if k not in ("defocusStrength", "bvhQuality")} == {k: v for k, v in sc.settings.items() if k not in ("defocusStrength", "bvhQuality")}


def test_sphere_masks_clear_bits_in_half_of_the_scenes_with_spheres(family):
    with_spheres = [s for s in cs.SEEDS if family[s]["scene"].spheres]
    cleared = [s for s in with_spheres if family[s]["sph"]["mean_mask"] < len(family[s]["scene"].spheres)]
    print(f"sphere masks with a cleared bit: {len(cleared)} of {len(with_spheres)} scenes: {cleared}")
    assert len(with_spheres) >= len(cs.SEEDS) // 2 and 2 * len(cleared) >= len(with_spheres)


def test_triangle_masks_clear_bits_in_half_of_the_scenes_with_triangles(family):
    with_tris = [s for s in cs.SEEDS if family[s]["scene"].models]
    cleared = [s for s in with_tris if family[s]["tri"]["mean_mask"] < sum(cs.triangle_counts(family[s]["scene"]))]
    print(f"triangle masks with a cleared bit: {len(cleared)} of {len(with_tris)} scenes: {cleared}")
    assert len(with_tris) >= len(cs.SEEDS) // 2 and 2 * len(cleared) >= len(with_tris)


def test_a_quarter_of_the_scenes_with_triangles_have_a_tile_with_an_empty_mask(family):
    with_tris = [s for s in cs.SEEDS if family[s]["scene"].models]
    empty = [s for s in with_tris if family[s]["tri"]["share0"] > 0]
    print(f"an empty triangle mask: {len(empty)} of {len(with_tris)} scenes: {empty}")
    assert 4 * len(empty) >= len(with_tris)
    assert len(cs.EMPTY_TRI_MASK_SEEDS) == 6 and set(cs.EMPTY_TRI_MASK_SEEDS) <= set(empty)


def test_no_oracle_image_of_the_family_holds_a_nan(family):
    assert [s for s in cs.SEEDS if not family[s]["finite"]] == []


def test_every_listed_case_occurs(pkg):
    scenes = {s: cs.scene(pkg, s)[0] for s in cs.SEEDS}
    assert {len(sc.spheres) for sc in scenes.values()} == {0, 1, 2, 3, 17, 31, 32}
    splits = {cs.triangle_counts(sc) for sc in scenes.values()}
    assert {(12, 2, 1, 1), (1, 1, 1, 13), ()} <= splits
    assert any(len(s) == 4 for s in splits) and any(sum(s) == 16 for s in splits) and {len(s) for s in splits} == {0, 1, 2, 3, 4}
    assert all(1 <= sum(s) <= 16 for s in splits if s)
    assert {sc.camera.fieldOfView for sc in scenes.values()} == {5.0, 30.0, 60.0, 90.0, 140.0}
    assert {sc.settings["divergeStrength"] for sc in scenes.values()} == {0.0, 1.5, 3.0, 50.0}
    assert {sc.settings["maxBounceCount"] for sc in scenes.values()} == {0, 1, 4, 9}
    assert {sc.settings["numRaysPerPixel"] for sc in scenes.values()} == {1, 2, 3}
    assert {sc.settings["useSky"] for sc in scenes.values()} == {False, True}
    assert any(sc.camera.transform.euler[2] != 0 for sc in scenes.values()) and any(sc.camera.transform.euler[2] == 0 for sc in scenes.values())
    assert all(abs(sc.camera.transform.euler[0]) <= 20 and abs(sc.camera.transform.euler[1]) <= 30 for sc in scenes.values())
    assert 2 * sum(1 for sc in scenes.values() if sc.width % 8 or sc.height % 8) > len(scenes), "mostly not multiples of 8"
    parts = [cs.partition_of(s) for s in cs.SEEDS if cs.partition_of(s)]
    assert 4 * len(parts) == len(cs.SEEDS) and {p[0] for p in parts} == {8, 16} and {p[2] for p in parts} == {2, 3} and all(0 <= p[1] < p[2] for p in parts)
    for s in cs.SEEDS:   # every part has rows
        p = cs.partition_of(s)
        if p:
            assert len(pkg.dist.global_rows_of(p[1], p[2], scenes[s].height, p[0])) > 0, s

    def camera_near(sc):   # inside a sphere or within 1 % of its surface
        o = np.array(sc.camera.transform.position)
        return any(np.linalg.norm(o - np.array(s.centre)) <= 1.01 * s.radius for s in sc.spheres)
    near = sum(1 for sc in scenes.values() if camera_near(sc))
    assert len(scenes) / 4 <= near <= len(scenes) / 2, near   # "roughly a third"

    def has_behind(sc):   # the whole line has a discriminant, both roots are negative
        o, f = np.array(sc.camera.transform.position), sc.camera.transform.forward
        return any(np.dot(np.array(s.centre) - o, f) < -s.radius and np.linalg.norm(np.cross(np.array(s.centre) - o, f)) < s.radius for s in sc.spheres)
    assert sum(1 for sc in scenes.values() if has_behind(sc)) >= 6
    assert sum(1 for sc in scenes.values() if any(a.centre == b.centre and a.radius == b.radius for a, b in zip(sc.spheres, sc.spheres[1:]))) >= 6
    glass = [m.material.flag == pkg.abi.MATERIAL_GLASS for sc in scenes.values() for m in sc.models]
    assert len(glass) / 4 <= sum(glass) <= len(glass) / 2   # "one third"
    scales = [m.transform.scale for sc in scenes.values() for m in sc.models]
    assert {sum(1 for v in s if v < 0) for s in scales} == {0, 1, 3}
    assert any(abs(s[0]) == 40 and abs(s[1]) == 40 and abs(s[2]) == 1 for s in scales)


def test_the_walks_make_every_kind_of_step(pkg):
    """the walks of tests/test_gpu_tile_fuzz.py::test_one_context_through_key_changing_calls are plain data: checked here, without a device"""
    kinds = [s["kind"] for seed in cs.WALK_SEEDS for s in cs._walk(pkg, seed)]
    assert any(s["kind"] == "model" and s["u"][10] < 0.5 for seed in cs.WALK_SEEDS for s in cs._walk(pkg, seed)), "no mirrored transform"
    assert set(kinds) == {"sphere", "model", "camera", "fov", "diverge", "defocus", "resize_same_tiles", "resize", "upload_in_cap",
                          "upload_over_a_cap", "upload_in_cap_again", "reset"}
    for seed in cs.WALK_SEEDS:
        k = [s["kind"] for s in cs._walk(pkg, seed)]
        assert len(k) == cs.STEPS and k.index("upload_over_a_cap") < k.index("upload_in_cap_again") and k.index("defocus") <= cs.STEPS - 3


def test_coverage_md_cites_test_functions_of_the_fuzz_files_that_exist():
    """COVERAGE.md cites the tests of this file and of tests/test_gpu_tile_fuzz.py with their path, a form tests/test_docs.py does not look at"""
    text = open(os.path.join(ROOT, "COVERAGE.md")).read()
    cited = set(re.findall(r"`tests/(test_(?:gpu_)?tile_fuzz\.py)::(test_[A-Za-z_0-9]+)", text))
    assert {f for f, _ in cited} == {"test_gpu_tile_fuzz.py"} and len(cited) >= 4
    assert "`tests/test_tile_fuzz.py`" in text and "`tests/capfuzz_scenes.py`" in text
    for f, fn in cited:
        assert re.search(r"^def %s\(" % re.escape(fn), open(os.path.join(ROOT, "tests", f)).read(), flags=re.M), (f, fn)
