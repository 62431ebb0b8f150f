"""The catalogue of tests/hazard_scenes.py on the CPU: before a planted value reaches the device, the oracle is pinned to the reference
text on it (rule 1), the expected image leaves something to compare (rule 2), the case changes something (rule 3) and every base scene
carries every hazard that applies to it, every guard has a case (rule 4).  tests/test_gpu_hazards.py renders the same catalogue on the GPU.

For the triangle and mesh cases, besides: the seen triangle is seen, each plant is what it is called, the `tables` column is primary_fill's
rule restated, the pairs the BVH builders refuse are refused by every builder, and the premises of the device half's threshold ray.

The reference legs (rule 1) need oracle/_ref, which build() compiles where the reference checkout is; they skip where it is absent and
fail where it is stale."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import hazard_scenes as hz
import host_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

ref_lib = graft._ref_lib()
IDS = [c.name for c in hz.CASES]


def _ref_or_none(pkg, variant, name):
    lib = ref_lib.load(pkg, variant)
    if lib is None:
        return None
    why = ref_lib.stale_reason([name])
    if why:
        pytest.fail("stale reference library: " + why)
    return lib


@pytest.fixture(scope="module")
def refs(pkg):
    return {"": _ref_or_none(pkg, "", "libref.so"), "spheres": _ref_or_none(pkg, "spheres", "libref_spheres.so")}


def _bases(case):
    """the bases a case renders on: those it applies to and builds on (test_refused_pairs_are_refused_by_every_builder has the others)"""
    return [b for b in hz.BASES if case.builds(b)]


# ---- the base scenes are what the catalogue says they are ------------------------------------------------------------------------------

def test_base_scenes_are_one_per_kernel_family(pkg, api, orc):
    info = {}
    for base in hz.BASES:
        rig = hz.Rig(pkg, orc, base)
        assert rig.w <= 48 and rig.h <= 32
        info[base] = (rig, api.validate_scene_arrays(rig.models, rig.triangles, rig.nodes, rig.spheres))
    rig, v = info["flat-tables"]   # within every cap of rt_primary.h
    assert v["flat"] == 1 and 2 <= len(rig.spheres) <= 32 and 2 <= len(rig.models) <= 4 and len(rig.triangles) <= 16 and rig.p.defocusStrength == 0.0
    rig, v = info["flat-general"]   # FLAT, above two caps: the general sphere loop (a second candidate word) and the unmasked triangle walk
    assert v["flat"] == 1 and len(rig.spheres) > 32 and len(rig.models) >= 2 and len(rig.triangles) > 16 and rig.w * rig.h >= 48 * 32
    rig, v = info["bvh"]
    assert v["flat"] == 0 and len(rig.models) <= 64 and len(rig.spheres) == 0
    rig, v = info["many"]
    assert v["flat"] == 0 and len(rig.models) > 64 and len(rig.spheres) > 0
    for base in hz.BASES:   # the targets exist, and every frame has bounces to plant materials in
        rig, t = info[base][0], hz.TARGETS[base]
        assert t.model < len(rig.models) and (t.sphere is None or t.sphere < len(rig.spheres)) and rig.p.maxBounceCount >= 1 and rig.p.numRaysPerPixel >= 1


@pytest.mark.parametrize("case", hz.CASES, ids=IDS)
def test_no_record_of_the_catalogue_is_refused(pkg, api, orc, case):
    """rt_validate_scene is the host half of rt_upload_scene and gives its status: every planted record is accepted, so no case is `refused`
    by the upload and every one has to render as the reference does.  The only refusals are the BVH builders', of two mesh cases on the
    bases where they have to split: a named outcome of Rig, with either builder"""
    assert case.refused is None or (case.kind == "mesh" and set(case.refused.values()) == {"build_bvh"})
    for base in hz.BASES:
        if not case.applies(base):
            continue
        for builder in (orc, api):
            rig = hz.Rig(pkg, builder, base, case)
            if not case.builds(base):
                assert rig.refused == ("build_bvh", pkg.abi.RT_ERR_SCENE), (case.name, base, rig.refused)
                continue
            assert rig.refused is None, (case.name, base, rig.refused)
            api.validate_scene_arrays(rig.models, rig.triangles, rig.nodes, rig.spheres)   # raises RtError on a refusal


def test_matrix_hazards_are_what_they_are_called(pkg, orc):
    rig = hz.Rig(pkg, orc, "bvh")
    l2w = hz._from_abi(rig.models[hz.TARGETS["bvh"].model]["localToWorld"])
    a, b = hz.matrix_pair(l2w, "singular")
    assert not a[0:3].any() and not b[[0, 4, 8, 12]].any() and np.isfinite(a).all() and np.isfinite(b).all()   # a zero column / a zero row
    for k in (1e-20, 1e15):
        a, b = hz.matrix_pair(l2w, k)
        assert np.isfinite(a).all() and np.isfinite(b).all() and a[:12].any() and b[:12].any()
        prod = hz._from_abi(a) @ hz._from_abi(b)
        assert np.allclose(prod, np.eye(4), atol=1e-5)
    a, b = hz.matrix_pair(l2w, "nan")
    assert np.isnan(a).sum() == 1 and np.isnan(b).sum() == 1


# ---- rule 1 ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", hz.CASES, ids=IDS)
def test_rule1_the_oracle_equals_the_reference_text(pkg, orc, refs, case):
    """images after 2 single frames and after 3 more, bit for bit under the NaN-position rule; segments and the reference's own two
    stats counters (triangle tests, box tests = inner steps)"""
    for base in _bases(case):
        lib = refs["spheres" if hz.TARGETS[base].sphere is not None else ""]
        if lib is None:
            pytest.skip("oracle/_ref is not here (built from the reference checkout)")
        tr = lib.create_tracer(8)
        try:
            got = hz.drive(hz.Rig(pkg, orc, base, case), tr)
        finally:
            tr.close()
        want = hz.expected(pkg, orc, base, case)
        for part, g, o in (("two single frames", got[0], want[0]), ("then 3 fused frames", got[1], want[1])):
            hz.assert_image(o[0], g[0], f"{case.name} on {base}, {part}: the oracle's AccumulatedRender != the reference text's")
            hz.assert_image(o[1], g[1], f"{case.name} on {base}, {part}: the oracle's FrameRender != the reference text's")
        for k in ("segments", "triTests", "innerSteps", "pixelFrames"):
            assert got[2][k] == want[2][k], (case.name, base, k, got[2][k], want[2][k])


# ---- rule 2 ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", hz.CASES, ids=IDS)
def test_rule2_the_expected_image_leaves_something_to_compare(pkg, orc, case):
    for base in _bases(case):
        want = hz.expected(pkg, orc, base, case)
        share = max(hz.nan_share(want[0][0]), hz.nan_share(want[1][0]))
        print(f"{case.name} on {base}: {share:.2f} of the pixels hold a NaN colour")
        assert case.saturating or share <= 0.75, (case.name, base, share)
        assert want[2]["pixelFrames"] == 5 * want[1][0].shape[0] * want[1][0].shape[1]


def test_rule2_saturating_cases_are_few_and_named():
    names = [c.name for c in hz.CASES if c.saturating]
    assert len(names) <= 3 and "sun-intensity-inf" in names, names


# ---- rule 3 ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", hz.CASES, ids=IDS)
def test_rule3_the_case_bites(pkg, orc, case):
    """on every base it applies to, the oracle's images or counters differ from the unplanted scene's; the one exception is a case on
    flat-tables whose `tables` is "off": there the device half asserts that the three tables went off"""
    for base in _bases(case):
        want, plain = hz.expected(pkg, orc, base, case), hz.expected(pkg, orc, base, None)
        differs = not all(hz.same_image(a, b) for k in (0, 1) for a, b in zip(want[k], plain[k])) or \
            any(want[2][k] != plain[2][k] for k in ("segments", "triTests", "innerSteps", "sphereTests", "modelVisits", "leafSteps"))
        flips = base == "flat-tables" and case.tables == "off"
        assert differs or flips, f"{case.name} on {base} changes nothing and flips nothing"


# ---- rule 4 ------------------------------------------------------------------------------------------------------------------------------

def test_rule4_every_base_carries_every_hazard_and_every_guard_has_a_case(pkg, orc):
    print("\n" + hz.table())
    print("saturating:", [c.name for c in hz.CASES if c.saturating], " refused:", [c.name for c in hz.CASES if c.refused is not None])
    for base in hz.BASES:
        rig = hz.Rig(pkg, orc, base)
        for c in hz.CASES:
            assert c.applies(base) == (c.kind != "sphere" or len(rig.spheres) > 0), (c.name, base)
    for g in hz.GUARDS:
        assert any(c.guard == g for c in hz.CASES), f"no case is aimed at {g}"
    kinds = {c.kind for c in hz.CASES}
    assert kinds == {"sphere", "model", "matrix", "material", "glass", "setting", "param", "triangle", "mesh"}
    # a glass hazard sets flag = 2, on the material the base scene plants in
    for c in hz.CASES:
        if c.kind == "glass":
            for base in hz.BASES:
                rig = hz.Rig(pkg, orc, base, c)
                t = hz.TARGETS[base]
                rec = rig.spheres[t.sphere] if t.material_on == "sphere" else rig.models[t.model]
                assert int(rec["material"]["flag"]) == 2, (c.name, base)
    # both table states occur among the cases the flat-tables base carries, for the guards that switch them
    assert {c.tables for c in hz.CASES if c.guard == "primary_fill"} == {"off"}
    assert {c.tables for c in hz.CASES if c.guard == "tile_cand_finite"} == {"on"}
    # the side passes: at least 12 values, every kind of object hazard; the NEE cases are the four emission and area hazards
    side = [hz.BY_NAME[n] for n in hz.SIDE_CASES]
    assert len(side) >= 12 and {c.kind for c in side} == {"sphere", "model", "matrix", "material", "glass", "triangle", "mesh"}
    assert set(hz.NEE_CASES) == {"emission-inf", "emission-1e38", "radius-0", "matrix-singular"}
    # the triangle values: both table states among the cases aimed at primary_fill's triangle entries and tile_tri_mask's keep rule; the
    # side passes, the layout run and the light table's area rule take named cases of both kinds / of the triangle kind, all of which
    # build on the bases they run on
    assert {c.tables for c in hz.CASES if c.guard in ("tri_primary", "tile_tri_finite")} == {"on", "off"}
    assert {"tri-coincident", "tri-vertex-1e20", "tri-vertex-nan", "tri-normals-zero", "tri-normals-opposed", "tri-tiny-1e-4", "mesh-vertex-nan",
            "mesh-flat"} <= set(hz.SIDE_CASES)
    assert all(hz.BY_NAME[n].builds(b) for n in hz.SIDE_CASES for b in hz.SIDE_BASES if hz.BY_NAME[n].applies(b))
    assert set(hz.NEE_TRI_CASES) == {"tri-degenerate", "tri-vertex-1e20", "tri-vertex-nan", "tri-tiny-1e-20"}
    assert set(hz.LAYOUT_CASES) == {"tri-vertex-1e20", "tri-coincident", "mesh-vertex-nan"} and set(hz.LAYOUT_BASES) == {"bvh", "many"}
    assert all(hz.BY_NAME[n].builds(b) for n in hz.LAYOUT_CASES for b in hz.LAYOUT_BASES)
    # a refusal is a builder's, of a mesh value, and never on a FLAT base (one leaf: nothing to split)
    for c in hz.CASES:
        assert not c.refused or (c.kind == "mesh" and c.guard == "bvh_build" and set(c.refused) <= {"bvh", "many"}), c.name


# ---- the triangle values -------------------------------------------------------------------------------------------------------------------

TRI = [c for c in hz.CASES if c.kind in ("triangle", "mesh")]
F = np.float32


def _cross(a, b):
    """fp32, one rounding per operation: (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x)"""
    with np.errstate(all="ignore"):
        return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                         a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1).astype(F)


def _face(T):
    with np.errstate(all="ignore"):
        return _cross(T["posB"] - T["posA"], T["posC"] - T["posA"])


def test_the_seen_triangle_is_seen(pkg, orc):
    """on every base the seen triangle is the first hit of at least SEEN_FLOOR = 4 pixel-centre rays of the unplanted scene (the floor
    tests/test_many_models.py uses for its witnesses), it lies in the triangle model's range, and oracle_ray_triangle named it"""
    assert hz.SEEN_FLOOR == 4
    for base in hz.BASES:
        t, rig = hz.aim(pkg, base), hz.Rig(pkg, orc, base)
        lo = int(rig.models["triOffset"][t.tri_model])
        print(f"{base}: {rig.w} x {rig.h}, triangle model {t.tri_model} ({int(rig.tri_count[t.tri_model])} triangles), seen triangle {t.seen}: "
              f"first hit of {t.seen_count} pixel-centre rays; the scene's most seen (model, triangle, rays): {t.most_seen[:4]}")
        assert lo <= t.seen < lo + int(rig.tri_count[t.tri_model])
        assert t.seen_count >= hz.SEEN_FLOOR, (base, t.seen_count)
        assert t.most_seen[0][2] >= t.seen_count and sum(c for _, _, c in t.most_seen) <= rig.w * rig.h


def test_triangle_plants_are_what_they_are_called(pkg, orc):
    """in fp32, on every base: the face AB x AC of the seen triangle is inf under tri-vertex-1e20 and finite (and huge) under
    tri-vertex-1e15; every face of the target model is exactly 0 under tri-degenerate and tri-tiny-1e-20 and is not under tri-tiny-1e-4;
    under tri-normals-opposed the interpolated normal is exactly 0 inside the triangle; only values were written"""
    for base in hz.BASES:
        plain, t = hz.Rig(pkg, orc, base), hz.aim(pkg, base)
        lo = int(plain.models["triOffset"][t.tri_model])
        mine = slice(lo, lo + int(plain.tri_count[t.tri_model]))

        def planted(name):
            rig = hz.Rig(pkg, orc, base, hz.BY_NAME[name])
            assert rig.models.tobytes() == plain.models.tobytes() and rig.nodes.tobytes() == plain.nodes.tobytes(), (name, base)
            assert len(rig.triangles) == len(plain.triangles) and plain.triangles.tobytes() == hz.Rig(pkg, orc, base).triangles.tobytes()
            other = np.ones(len(plain.triangles), dtype=bool)
            other[mine] = False
            assert rig.triangles[other].tobytes() == plain.triangles[other].tobytes(), (name, base)
            return rig.triangles
        f = _face(planted("tri-vertex-1e20")[t.seen:t.seen + 1])[0]
        assert np.isinf(f).any() and not np.isnan(f).any(), (base, f)
        f = _face(planted("tri-vertex-1e15")[t.seen:t.seen + 1])[0]
        assert np.isfinite(f).all() and np.abs(f).max() > 1e12, (base, f)
        for name in ("tri-vertex-nan", "tri-vertex-inf"):
            assert not np.isfinite(_face(planted(name)[t.seen:t.seen + 1])).all(), (name, base)
        for name in ("tri-degenerate", "tri-tiny-1e-20"):
            assert not _face(planted(name)[mine]).any(), (name, base)
        f = _face(planted("tri-tiny-1e-4")[mine])
        assert np.isfinite(f).all() and f.any(axis=1).all(), base
        T = planted("tri-normals-opposed")[mine]
        # w * normA + u * normB + v * normC at u = v = 1/4, w = 1/2 (all exact in fp32): 0 exactly, whatever normA is
        with np.errstate(all="ignore"):
            n = T["normA"] * F(0.5) + T["normB"] * F(0.25) + T["normC"] * F(0.25)
        assert not n.any() and T["normA"].any(axis=1).all(), base
        for name, k in (("tri-normals-1e20", np.inf), ("tri-normals-1e-30", 0.0)):
            T = planted(name)[mine]
            with np.errstate(all="ignore"):
                sq = (T["normA"] * T["normA"]).sum(axis=1, dtype=F)
            assert (sq == F(k)).all(), (name, base, sq)
        T = planted("tri-coincident")[mine]
        for i in range(1, len(T), 2):
            assert all(np.array_equal(T[p][i], T[p][i - 1]) for p in hz.POS) and all(np.array_equal(T[n][i], -T[n][i - 1]) for n in hz.NORM)


def test_determinant_at_the_threshold_premises(pkg, orc):
    """hazard_scenes.threshold_rig on every base, with the oracle: the ray's determinant is the float below 1E-8f, 1E-8f itself and the
    float above it; RC:206's `determinant >= 1E-8` keeps the last two (a hit 0.01 away, front face) and drops the first.  The device half
    is tests/test_gpu_hazards.py::test_determinant_exactly_at_the_threshold"""
    edges = hz.threshold_edges()
    assert [F(a * b) for a, b in (edges[k] for k in ("below", "at", "above"))] == [np.nextafter(hz.EPS, F(0)), hz.EPS, np.nextafter(hz.EPS, F(1))]
    out6, out10, F3 = (C.c_float * 6)(), (C.c_float * 10)(), C.c_float * 3
    for base in hz.BASES:
        for which, (s1, s2) in edges.items():
            rig, o, d = hz.threshold_rig(pkg, orc, base, s1, s2)
            T = rig.triangles[int(rig.models["triOffset"][0])]
            face = _face(rig.triangles[int(rig.models["triOffset"][0]):][:1])[0]
            assert face[0] == 0 and face[1] == 0 and face[2] == F(s1 * s2), (base, which, face)
            orc.ray_triangle(F3(*o[0]), F3(*d[0]), np.array([T]).ctypes.data, 1, out6)
            ot = orc.create_tracer(1)
            try:
                rig.upload(ot)
                orc.ray_collision(ot.h, F3(*o[0]), F3(*d[0]), out10)
            finally:
                ot.close()
            near = out10[0] != 0 and abs(out10[2] - 0.01) < 1e-4
            print(f"{base}, determinant {which} 1E-8f: oracle_ray_triangle didHit {out6[0]}, the scene's hit at {out10[2] if out10[0] else None}")
            assert (out6[0] != 0) == (which != "below") and near == (which != "below"), (base, which)
            if near:
                assert out10[1] == 0 and out10[2] == out6[2]


def _reasoned_tables(rig):
    """primary_fill's rule for the triangle entries (rt_primary.h), restated in fp32 from the records: lpos = worldToLocal * o summed left
    to right, vro = lpos - A, d = dot(vro, AB x AC); "on" iff every lpos, vro and d is finite"""
    o = np.array(list(rig.p.camLocalToWorld), dtype=F)[12:15]
    fin = True
    with np.errstate(all="ignore"):
        for mi in range(len(rig.models)):
            w = rig.models["worldToLocal"][mi]
            lpos = np.array([((w[r] * o[0] + w[4 + r] * o[1]) + w[8 + r] * o[2]) + w[12 + r] * F(1) for r in range(3)], dtype=F)
            lo = int(rig.models["triOffset"][mi])
            T = rig.triangles[lo:lo + int(rig.tri_count[mi])]
            vro, face = (lpos - T["posA"]).astype(F), _face(T)
            d = ((vro[:, 0] * face[:, 0] + vro[:, 1] * face[:, 1]) + vro[:, 2] * face[:, 2]).astype(F)
            fin = fin and bool(np.isfinite(lpos).all() and np.isfinite(vro).all() and np.isfinite(d).all())
    return "on" if fin else "off"


@pytest.mark.parametrize("case", TRI, ids=[c.name for c in TRI])
def test_tables_column_of_the_triangle_cases_is_reasoned(pkg, orc, case):
    """the `tables` column against primary_fill's rule restated on the flat-tables records (never read off the device); the unplanted
    base is `on`"""
    assert _reasoned_tables(hz.Rig(pkg, orc, "flat-tables")) == "on"
    assert case.builds("flat-tables")
    assert _reasoned_tables(hz.Rig(pkg, orc, "flat-tables", case)) == case.tables, case.name


@pytest.fixture(scope="module")
def tile_tri_driver(tmp_path_factory):
    """tests/tile_tri_driver.cpp as tests/test_tile_fuzz.py builds it: a stand-alone program under the address and undefined-behaviour
    sanitizers"""
    d = tmp_path_factory.mktemp("hazard_tiles")
    exe = host_driver.build(d, "tile_tri", ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                            "-static-libasan", "-static-libubsan"], exe="tile_tri_san")
    return d, exe


def _write_triangle_scene(pkg, rig, path):
    """capfuzz_scenes.write_triangle_scene from a Rig's (planted) arrays: the driver's text form"""
    p = rig.p
    lines = [f"{rig.w} {rig.h} 8 0 1 {p.divergeStrength!r}", " ".join(repr(float(v)) for v in p.camLocalToWorld),
             " ".join(repr(float(v)) for v in p.viewParams), str(len(rig.models))]
    for i in range(len(rig.models)):
        m, root = rig.models["worldToLocal"][i], rig.nodes[int(rig.models["nodeOffset"][i])]
        n = int(root["triangleCount"])
        assert n > 0
        lines.append(" ".join(repr(float(m[c * 4 + r])) for r in range(3) for c in range(4)))
        lines.append(f"{int(int(rig.models['material']['flag'][i]) != pkg.abi.MATERIAL_GLASS)} {n}")
        first = int(rig.models["triOffset"][i]) + int(root["startIndex"])
        for t in rig.triangles[first:first + n]:
            lines.append(" ".join(repr(float(v)) for v in (*t["posA"], *t["posB"], *t["posC"])))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path


@pytest.mark.parametrize("case", [None] + TRI, ids=["unplanted"] + [c.name for c in TRI])
def test_tile_tri_mask_keeps_every_planted_triangle_a_ray_accepts(pkg, orc, tile_tri_driver, case):
    """tile_tri_mask's keep rule ("any value that is not finite", "a degenerate triangle") through the host driver's existing scene
    input: on the flat-tables records of every triangle and mesh case, in every tile, every triangle that accepts a ray of the kernel's
    own raygen under tri_test's arithmetic has its bit (misses=0), with the sanitizers on"""
    import re
    import subprocess
    d, exe = tile_tri_driver
    rig = hz.Rig(pkg, orc, "flat-tables", case)
    path = _write_triangle_scene(pkg, rig, str(d / f"{case.name if case else 'unplanted'}.txt"))
    env = {k: v for k, v in os.environ.items() if not k.startswith("RT_")}
    p = subprocess.run([exe, "scene", path, "1"], capture_output=True, env=env, timeout=600)
    out = p.stdout.decode(errors="replace")
    last = (out.strip().splitlines() or [""])[-1]
    print(f"{case.name if case else 'unplanted'}: {last}")
    assert p.returncode == 0 and last.startswith("ok ") and " misses=0 " in last + " ", (p.returncode, out[-2000:], p.stderr.decode(errors="replace")[-2000:])
    figures = {k: float(v) for k, v in re.findall(r"(\w+)=([-0-9.e+]+)", last)}
    assert figures["triangles"] == len(rig.triangles) and figures["checked"] == figures["tiles"] > 0


REFUSED = [(c, b) for c in hz.CASES for b in hz.BASES if c.kind == "mesh" and c.guard == "bvh_build" and c.applies(b)]


@pytest.mark.parametrize("case,base", REFUSED, ids=[f"{c.name}-{b}" for c, b in REFUSED])
def test_refused_pairs_are_refused_by_every_builder(pkg, api, orc, case, base):
    """the planted mesh through rt_build_bvh, rt_build_bvh_mt on 5 threads, the oracle's builder and the reference's BVH.cs text
    (oracle/_ref/libref_bvh.so): where the catalogue says refused all refuse with RT_ERR_SCENE, elsewhere all build the same bytes"""
    ref = ref_lib.load_bvh(pkg)
    if ref is not None:
        why = ref_lib.stale_reason(["libref_bvh.so"])
        if why:
            pytest.fail("stale reference library: " + why)
    rig = hz.Rig(pkg, orc, base, case)
    mesh = rig.meshes[hz.TARGETS[base].tri_model]
    assert not np.isfinite(mesh.vertices).all() or np.abs(mesh.vertices).max() >= F(3e19)
    builders = [("rt_build_bvh", api.build_bvh_arrays), ("rt_build_bvh_mt, 5 threads", lambda *a: api.build_bvh_arrays_mt(*a, 5)),
                ("oracle_build_bvh", orc.build_bvh_arrays)] + ([("BVH.cs", ref.build_bvh_arrays)] if ref is not None else [])
    outcomes = []
    for name, build in builders:
        try:
            nodes, tris, stats = build(mesh.vertices, mesh.normals, mesh.triangles, rig.bvh_quality)   # the base scene's own quality
            stats = dict(stats)
            stats.pop("timeMs")
            outcomes.append((name, "built", nodes.tobytes(), tris.tobytes(), stats))
        except pkg.abi.RtError as e:
            outcomes.append((name, "refused", e.status))
    print(f"{case.name} on {base}: " + ", ".join(f"{o[0]}: {o[1]}" for o in outcomes))
    for o in outcomes:
        assert o[1:] == outcomes[0][1:], (case.name, base, o[0], "differs from", outcomes[0][0])
    if case.builds(base):
        assert outcomes[0][1] == "built"
    else:
        assert outcomes[0][1:] == ("refused", pkg.abi.RT_ERR_SCENE)
    if ref is None:
        pytest.skip("oracle/_ref/libref_bvh.so is not here (built from the reference checkout): the other three builders agree")
