"""The catalogue of tests/hazard_scenes.py on the CPU: before a planted value reaches the device, the oracle is pinned to the reference
text on it (rule 1), the expected image leaves something to compare (rule 2), the case changes something (rule 3) and every base scene
carries every hazard that applies to it, every guard has a case (rule 4).  tests/test_gpu_hazards.py renders the same catalogue on the GPU.

The reference legs (rule 1) need oracle/_ref, which build() compiles where the reference checkout is; they skip where it is absent and
fail where it is stale."""
import os
import sys

import numpy as np
import pytest

import hazard_scenes as hz

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
    return [b for b in hz.BASES if case.applies(b)]


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
    and every one has to render as the reference does"""
    assert case.refused is None
    for base in _bases(case):
        rig = hz.Rig(pkg, orc, base, case)
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
    assert kinds == {"sphere", "model", "matrix", "material", "glass", "setting", "param"}
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
    assert len(side) >= 12 and {c.kind for c in side} == {"sphere", "model", "matrix", "material", "glass"}
    assert set(hz.NEE_CASES) == {"emission-inf", "emission-1e38", "radius-0", "matrix-singular"}
