"""Non-finite and extreme scene values on every kernel: the catalogue of tests/hazard_scenes.py on the GPU.  tests/test_hazards.py has
pinned the oracle to the reference text on every case on the CPU; here the device renders each case and must equal the oracle.

Whole frames (every case, every base scene it applies to; the shipped and the STATS instantiation): both images after two single frames
and after a fused launch of three, under the NaN-position rule; segments and pixelFrames, in the STATS build all seven exact counters;
filter_violations == 0; the three rt_debug_* calls after either part say what the catalogue reasons (`tables`: (1, 1, 1) or (0, 0, 0) on
flat-tables, (0, 0, 0) on every other base).  The watchdog word: a context whose watchdog fired fails every pixel read and
rt_get_counters with RT_ERR_HIP (the wrapper raises), so the reads of each case succeeding IS that assertion.  What no debug call exposes — a
per-tile table that keeps every bit, the root filter dropped for one model — is held by the image, the exact counters and the audit.

The contexts are shared by the cases of this module (a case starts with rt_resize, rt_upload_scene, rt_set_params and
rt_reset_accumulation): a table left over from the previous case's key would show as a wrong pixel.

Side passes (hazard_scenes.SIDE_CASES on SIDE_BASES): rt_render_aov, rt_query_closest / rt_query_occluded / rt_debug_intersect,
rt_radiance_trace and (NEE_CASES) rt_nee_trace and rt_mis_trace against the oracle's functions.  Floats are compared bit for bit, except that where
the expected value is a NaN the device's must be one too (a NaN's sign and payload are not part of the contract).

The triangle and mesh cases ride through all of the above; on top, for them: (object, triangle) of the AOV and query records is the
triangle oracle_ray_triangle names; rays at the corners and edges of the most seen triangles and one at tri_test's determinant threshold
exactly; three cases under the layout that moves and pre-differences the triangle records; the light table's area rule with an emissive
model of planted triangles; rt_build_bvh_gpu_batch on every planted mesh.  Only values are planted: every index, count and offset stays
what validation accepted."""
import copy
import ctypes as C
import time

import numpy as np
import pytest

import aov_support as ta
import hazard_scenes as hz
import mis_reference as mr
import nee_reference as nr
import radiance_reference as rr
from gpu_support import KEYS, environment

pytestmark = pytest.mark.gpu
F = np.float32
F3 = C.c_float * 3
ENV = ("RT_TILE_TRI", "RT_TILE_CAND", "RT_PRIMARY", "RT_POOL", "RT_POOL_MIN_ITEMS")   # the variables tests/test_gpu_tile_tri.py clears
POOLED, SINGLE = {"RT_POOL_MIN_ITEMS": "0"}, {"RT_POOL": "0"}
ALL = [None] + hz.CASES
IDS = ["unplanted"] + [c.name for c in hz.CASES]


@pytest.fixture(scope="module")
def contexts(api):
    """(name, environment, tracer, stats?) — made once: the default schedule, and for flat-general pooled workgroups / single waves"""
    made = []
    for name, env in (("default", {}), ("pooled", POOLED), ("single waves", SINGLE)):
        for stats in (False, True):
            with environment(env, ENV) if env else _nothing():
                tr = api.create_tracer(0)
            tr.enable_stats(stats)
            made.append((name, env, tr, stats))
    yield made
    for _, _, tr, _ in made:
        tr.close()


class _nothing:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def _tables(tr):
    return (tr.primary_table(), tr.tile_cand(), tr.tile_tri())


def _drive_watched(rig, tr):
    """hz.drive, and what the three debug calls say after the single frames and after the fused launch"""
    rig.upload(tr)
    for i in range(2):
        tr.set_params(rig.params(i))
        tr.render_frame()
    single = (tr.read_accumulated().copy(), tr.read_frame().copy())
    after_single = _tables(tr)
    tr.set_params(rig.params(2))
    tr.render_frames(3)
    fused = (tr.read_accumulated().copy(), tr.read_frame().copy())
    return single, fused, tr.counters(), (after_single, _tables(tr))


def _check(pkg, api, orc, case, base, name, env, tr, stats):
    what = f"{case.name if case else 'unplanted'} on {base} ({name}, {'STATS' if stats else 'shipped'})"
    want = hz.expected(pkg, orc, base, case)
    with environment(env, ENV) if env else _nothing():
        tr.reset_counters()
        single, fused, c, debug = _drive_watched(hz.Rig(pkg, api, base, case), tr)
        viol = tr.phase_profile()["filter_violations"][0] if stats else 0
    print(f"{what}: segments {c['segments']} (oracle {want[2]['segments']}), tables {debug}, NaN share {hz.nan_share(want[1][0]):.2f}")
    for part, g, o in (("two single frames", single, want[0]), ("then 3 fused frames", fused, want[1])):
        hz.assert_image(g[0], o[0], f"{what}, {part}: AccumulatedRender != oracle")
        hz.assert_image(g[1], o[1], f"{what}, {part}: FrameRender != oracle")
    assert (c["segments"], c["pixelFrames"]) == (want[2]["segments"], want[2]["pixelFrames"]), (what, c, want[2])
    if stats:
        assert [c[k] for k in KEYS] == [want[2][k] for k in KEYS], (what, c, want[2])
        assert viol == 0, what
    on = base == "flat-tables" and (case is None or case.tables == "on")
    assert debug == (((1, 1, 1),) * 2 if on else ((0, 0, 0),) * 2), f"{what}: rt_debug_primary_table / _tile_cand / _tile_tri = {debug}"


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_every_case_on_every_base_equals_the_oracle(pkg, api, orc, contexts, case):
    bases = [b for b in hz.BASES if case is None or case.builds(b)]   # (a pair the builders refuse: test_gpu_builder_on_every_mesh_case)
    for base in bases:
        hz.expected(pkg, orc, base, case)   # (the oracle's renders, on the CPU: not part of the time printed below)
    t0 = time.perf_counter()
    for base in bases:
        for name, env, tr, stats in contexts:
            if name == "default":
                _check(pkg, api, orc, case, base, name, env, tr, stats)
    print(f"{len(bases)} bases x 2 instantiations x 5 frames: {time.perf_counter() - t0:.2f} s on the device side")


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_flat_general_as_pooled_workgroups_and_as_single_waves(pkg, api, orc, contexts, case):
    assert case is None or case.applies("flat-general")
    for name, env, tr, stats in contexts:
        if name != "default":
            _check(pkg, api, orc, case, "flat-general", name, env, tr, stats)


# ---- the side passes ------------------------------------------------------------------------------------------------------------------

def _same(got, want):
    """bit for bit; where the expected float is a NaN, a NaN"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if want.dtype != np.float32:
        return got == want
    nan = np.isnan(want)
    return np.where(nan, np.isnan(got), got.view(np.uint32) == want.view(np.uint32))


def _assert_fields(got, want, fields, what):
    for f in fields:
        ok = _same(got[f], want[f])
        bad = np.argwhere(~ok.reshape(len(got), -1).all(axis=1))
        assert not len(bad), f"{what}: field {f}: {len(bad)} records differ; first {int(bad[0][0])}: got {got[int(bad[0][0])]}, want {want[int(bad[0][0])]}"


def _oracle_hits(orc, ot, origins, dirs):
    """oracle_ray_collision per ray: (n, 10) float32 = didHit, isBackface, dst, normal, pos, material flag"""
    out = np.zeros((len(origins), 10), dtype=F)
    o10 = (C.c_float * 10)()
    for i in range(len(origins)):
        orc.ray_collision(ot.h, F3(*origins[i]), F3(*dirs[i]), o10)
        out[i] = o10[:]
    return out


def _hit_records(abi, dtype, hits10):
    """the float fields and the hit word of RtRayHit / RtPixelAov records from oracle_ray_collision's answers (a miss: dst alone)"""
    want = np.zeros(len(hits10), dtype=dtype)
    hit = hits10[:, 0] != 0
    want["dst"] = hits10[:, 2]
    want["normal"][hit], want["pos"][hit] = hits10[hit, 3:6], hits10[hit, 6:9]
    glass = hits10[:, 9].astype(np.int64) == abi.MATERIAL_GLASS
    want["hit"][hit] = (np.where(glass, 2, 1) | np.where(hits10[:, 1] != 0, abi.AOV_HIT_BACKFACE, 0))[hit]
    return want, hit


def _side_setup(pkg, api, orc, contexts, base, case):
    rig = hz.Rig(pkg, api, base, case)
    tr = next(t for name, _, t, stats in contexts if name == "default" and not stats)
    rig.upload(tr)
    ot = orc.create_tracer(1)
    hz.Rig(pkg, orc, base, case).upload(ot)
    return rig, tr, ot


def _assert_named(pkg, orc, rig, origins, dirs, hits10, objects, triangles, what):
    """the device's (object, triangle) of every ray is one the oracle's hit can be (hazard_scenes.hit_candidates: oracle_ray_triangle over
    every model's range gives the hit's dst bit for bit): THE one where there is one; of a tie — coincident triangles, a shared edge —
    the walk order decides, and the record's normal and backface bit, compared with the oracle's elsewhere, say which.
    -> (rays named, ties among them)"""
    _, cands = hz.hit_candidates(pkg, orc, rig, np.ascontiguousarray(origins, dtype=F), np.ascontiguousarray(dirs, dtype=F), hits10)
    named = ties = 0
    for i, c in enumerate(cands):
        if c:
            got = (int(objects[i]) - rig.n_spheres, int(triangles[i]))
            assert got in c, f"{what}: ray {i}: (model, triangle) {got}, the oracle's hit is on {c}"
            named, ties = named + 1, ties + (len(c) > 1)
    return named, ties


SIDE = [hz.BY_NAME[n] for n in hz.SIDE_CASES]


@pytest.mark.parametrize("case", SIDE, ids=hz.SIDE_CASES)
def test_aov_records_of_a_hazard_scene(pkg, api, orc, contexts, case):
    """rt_render_aov, frame 2: every field of every pixel.  dst / normal / pos / hit from oracle_ray_collision on the camera rays of
    tests/test_gpu_aov.py; albedo from oracle_material_colour (a hit; the material is the one of the record's own object, whose flag
    must be the oracle's hit's) or oracle_environment_light (a miss); emission = emissionCol * emissionStrength; object and
    triangle: -1 exactly on a miss, a sphere's triangle -1, a model's inside the model's range."""
    abi = pkg.abi
    for base in hz.SIDE_BASES:
        if not case.applies(base):
            continue
        rig, tr, ot = _side_setup(pkg, api, orc, contexts, base, case)
        try:
            p = rig.params(1)
            aov = tr.render_aov(rig.frame0 + 1).reshape(-1)
            o, d = ta.camera_rays(orc, p, rig.w, rig.h, rig.frame0 + 1)
            o, d = o.reshape(-1, 3), d.reshape(-1, 3)
            hits10 = _oracle_hits(orc, ot, o, d)
            want, hit = _hit_records(abi, abi.AOV_DTYPE, hits10)
            what = f"{case.name} on {base}: rt_render_aov"
            assert np.array_equal(aov["object"] >= 0, hit), what + ": object >= 0 exactly where the oracle hits"
            o3 = F3()
            for i in range(len(aov)):
                if hit[i]:
                    obj = int(aov["object"][i])
                    mat = rig.materials[obj:obj + 1].copy()
                    assert int(mat["flag"][0]) == int(hits10[i, 9]), (what, i, obj)
                    orc.material_colour(mat.ctypes.data, F3(*hits10[i, 6:9]), F3(*hits10[i, 3:6]), 0, o3)
                    want["albedo"][i] = o3[:]
                    with np.errstate(all="ignore"):
                        want["emission"][i] = mat["emissionCol"][0][:3] * mat["emissionStrength"][0]
                elif p.useSky:
                    orc.environment_light(C.byref(p), F3(*d[i]), o3)
                    want["albedo"][i] = o3[:]
            _assert_fields(aov, want, ("dst", "normal", "pos", "hit", "albedo", "emission"), what)
            model = aov["object"] >= rig.n_spheres
            assert ((aov["triangle"] >= 0) == model).all(), what
            for i in np.argwhere(model).ravel():
                mi = int(aov["object"][i]) - rig.n_spheres
                off = int(rig.models["triOffset"][mi])
                assert off <= int(aov["triangle"][i]) < off + int(rig.tri_count[mi]), (what, i)
            if case.kind in ("triangle", "mesh"):   # object and triangle are the oracle's, named by oracle_ray_triangle
                named = _assert_named(pkg, orc, rig, o, d, hits10, aov["object"], aov["triangle"], what)
                print(f"{what}: (object, triangle) named for {named[0]} pixels, {named[1]} of them ties")
            print(f"{what}: {int(hit.sum())} of {len(hit)} pixels hit, {int(np.isnan(hits10).any(axis=1).sum())} records with a NaN")
        finally:
            ot.close()


@pytest.mark.parametrize("case", SIDE, ids=hz.SIDE_CASES)
def test_ray_queries_into_a_hazard_scene(pkg, api, orc, contexts, case):
    """one ray per pixel centre: rt_query_closest and rt_debug_intersect against oracle_ray_collision; rt_query_occluded at tmax = +inf
    (any hit), at the ray's own hit distance d (the comparison is strict: 0) and one ulp above it (1 where there is a hit)"""
    abi = pkg.abi
    for base in hz.SIDE_BASES:
        if not case.applies(base):
            continue
        rig, tr, ot = _side_setup(pkg, api, orc, contexts, base, case)
        try:
            o, d = hz.pixel_centre_rays(rig)
            o, d = o.reshape(-1, 3), d.reshape(-1, 3)
            hits10 = _oracle_hits(orc, ot, o, d)
            want, hit = _hit_records(abi, abi.RAYHIT_DTYPE, hits10)
            what = f"{case.name} on {base}"
            got = tr.query_closest(abi.make_rays(o, d))
            assert np.array_equal(got["object"] >= 0, hit), what + ": rt_query_closest: object >= 0 exactly where the oracle hits"
            _assert_fields(got, want, ("dst", "normal", "pos", "hit"), what + ": rt_query_closest")
            if case.kind in ("triangle", "mesh"):
                _assert_named(pkg, orc, rig, o, d, hits10, got["object"], got["triangle"], what + ": rt_query_closest")
            dbg = tr.debug_intersect(o, d)
            ok = _same(dbg, hits10)
            ok[~hit, 3:] = True   # (a miss: didHit, isBackface and dst are the contract)
            assert ok.all(), f"{what}: rt_debug_intersect: {int((~ok.all(axis=1)).sum())} rays differ from oracle_ray_collision"
            dst = hits10[:, 2]
            with np.errstate(all="ignore"):
                for name, tmax in (("+inf", np.full(len(o), np.inf, dtype=F)), ("d", dst), ("one ulp above d", np.nextafter(dst, F(np.inf)))):
                    occ = tr.query_occluded(abi.make_rays(o, d, tmax))
                    expect = (hit & (dst < tmax)).astype(np.uint32)
                    assert np.array_equal(occ, expect), f"{what}: rt_query_occluded at tmax = {name}: {int((occ != expect).sum())} rays differ"
            print(f"{what}: {int(hit.sum())} of {len(hit)} rays hit")
        finally:
            ot.close()


@pytest.mark.parametrize("case", SIDE, ids=hz.SIDE_CASES)
def test_radiance_of_camera_rays_into_a_hazard_scene(pkg, api, orc, contexts, case):
    """rt_radiance_trace of (camera ray 0 of frame 2, the generator state behind its two draws), one ray per pixel, at one ray per
    pixel in the parameters: oracle_trace_pixel of that frame (x / 1 is x)"""
    abi = pkg.abi
    for base in hz.SIDE_BASES:
        if not case.applies(base):
            continue
        rig, tr, ot = _side_setup(pkg, api, orc, contexts, base, case)
        try:
            frame = rig.frame0 + 1
            rig.p.numRaysPerPixel = 1
            p = rig.params(1)
            tr.set_params(p)
            ot.set_params(p)
            o, d, state = rr.camera_rays(orc, p, rig.w, rig.h, frame=frame)
            got = tr.radiance_trace(abi.make_path_rays(o.reshape(-1, 3), d.reshape(-1, 3), state.ravel()))
            want = rr.oracle_pixels(orc, ot, rig.w, rig.h, frame).reshape(-1, 3)
            ok = _same(got["rgb"], want).all(axis=1)
            assert ok.all(), f"{case.name} on {base}: rt_radiance_trace: {int((~ok).sum())} of {len(ok)} rays differ from oracle_trace_pixel"
            print(f"{case.name} on {base}: {int(np.isnan(want).any(axis=1).sum())} of {len(want)} rays carry a NaN")
        finally:
            ot.close()


def _nee_rig(pkg, api, base, name):
    """the four emission and area hazards: the object the value is planted in is made an emitter where the case does not do so itself"""
    case = hz.BY_NAME[name]
    t = hz.TARGETS[base]

    def scene(pkg_, sc, t_):
        if case.scene:
            case.scene(pkg_, sc, t_)
        if name == "radius-0":
            m = sc.spheres[t_.sphere].material
            m.flag, m.emissionCol, m.emissionStrength = 0, (1.0, 0.9, 0.7, 1.0), 5.0
        if name == "matrix-singular":
            m = sc.models[t_.model].material
            m.flag, m.emissionCol, m.emissionStrength = 0, (1.0, 0.9, 0.7, 1.0), 5.0
    made = hz.Case(name + "-emitter", case.kind, case.guard, case.tables, scene=scene, records=case.records)
    return hz.Rig(pkg, api, base, made), (t.sphere if name == "radius-0" else None)


def _emission_and_area_hazards(pkg, api, orc, contexts, name, estimator, trace, call):
    """The body of the NEE test below, for either light-sampling pass: `estimator` the reference's class, `trace` the tracer's method
    by name, `call` the C function for the messages.  Yields, per base, what a caller asserts more from:
    (what, rig, the planted object, the numpy table, the estimator with its logs, the expected records)"""
    abi = pkg.abi
    for base in hz.SIDE_BASES:
        if not hz.BY_NAME[name].applies(base):
            continue
        rig, zero_sphere = _nee_rig(pkg, api, base, name)
        tr = next(t for n, _, t, stats in contexts if n == "default" and not stats)
        rig.upload(tr)
        what = f"{name} on {base}"
        want = nr.light_table(abi, rig.models, rig.triangles, rig.spheres)
        got = api.light_table_arrays(rig.models, rig.triangles, rig.spheres)
        assert got["entries"].tobytes() == want["entries"].tobytes() and got["cdf"].tobytes() == want["cdf"].tobytes(), what
        counts = (want["n_sphere_entries"], want["n_triangle_entries"])
        assert (got["n_sphere_entries"], got["n_triangle_entries"]) == counts and tr.nee_light_count() == counts, what
        t = rig.targets
        planted = t.sphere if (t.material_on == "sphere" and name.startswith("emission")) or name == "radius-0" else rig.n_spheres + t.model
        if name in ("emission-inf", "radius-0"):   # excluded by the header's rules
            assert not want["in_table"][planted], what
        else:
            assert want["in_table"][planted], what
        assert np.isfinite(want["cdf"]).all() and np.isfinite(want["entries"]["prob"]).all()
        rig.p.numRaysPerPixel = 1
        p = rig.params(1)
        tr.set_params(p)
        o, d, state = rr.camera_rays(orc, p, rig.w, rig.h, frame=rig.frame0 + 1)
        rays = abi.make_path_rays(o.reshape(-1, 3), d.reshape(-1, 3), state.ravel())[::7]
        est = estimator(pkg, orc, tr, rig.models, rig.triangles, rig.spheres, p)
        expect = est.trace(rays)
        out = getattr(tr, trace)(rays)
        ok = _same(out["rgb"], expect["rgb"]).all(axis=1) & (out["rng"] == expect["rng"])
        print(f"{what}: lights {counts}, {est.samples} samples, {est.shadow_rays} shadow rays, {est.unshadowed} unshadowed")
        assert ok.all(), f"{what}: {call}: {int((~ok).sum())} of {len(ok)} rays differ from the restated estimator"
        yield what, rig, planted, want, est, expect


@pytest.mark.parametrize("name", hz.NEE_CASES)
def test_nee_with_emission_and_area_hazards(pkg, api, orc, contexts, name):
    """rt_debug_light_table against the numpy table of tests/nee_reference.py, bit for bit; rt_nee_light_count; the header's rules leave
    out an emitter whose emission is not finite and a sphere of radius 0 (asserted); rt_nee_trace on every 7th pixel's camera ray against
    the estimator restated in tests/nee_reference.py"""
    assert len(list(_emission_and_area_hazards(pkg, api, orc, contexts, name, nr.Estimator, "radiance_trace_nee", "rt_nee_trace"))) >= 2


def _not_vacuous(what, est, expect, t0):
    """the two conditions that keep a MIS hazard case from passing on nothing, measured on the reference: at least a quarter of the
    compared records are finite and not zero, and samples were taken"""
    rgb = expect["rgb"]
    live = int((np.isfinite(rgb).all(axis=1) & (rgb != 0).any(axis=1)).sum())
    rules = {r: sum(1 for e in est.emission_log if e[3] == r) for r in sorted({e[3] for e in est.emission_log})}
    print(f"{what}: {live} of {len(rgb)} records finite and not zero, {int((~np.isfinite(rgb)).any(axis=1).sum())} not finite; {est.samples} samples, "
          f"{len(est.sample_log)} shadow rays, g == 0 in {sum(1 for s in est.sample_log if s[2] == 0.0)}; emissions behind a sample {rules}; "
          f"{time.perf_counter() - t0:.2f} s for this base, the reference included")
    assert 4 * live >= len(rgb), f"{what}: only {live} of {len(rgb)} compared records are finite and not zero"
    assert est.samples > 0, what
    mr.rules_allowed(est, what)


def _assert_map(pkg, api, what, rig):
    """rt_debug_light_map == tests/mis_reference.py::map_arrays, bit for bit -> (objects, words)"""
    objects, words, table = mr.map_arrays(pkg.abi, rig.models, rig.triangles, rig.spheres)
    got = api.light_map_arrays(rig.models, rig.triangles, rig.spheres)
    assert got["objects"].tobytes() == objects.tobytes() and got["triangles"].tobytes() == words.tobytes() and got["n_entries"] == len(table["entries"]), what
    return objects, words


@pytest.mark.parametrize("name", hz.NEE_CASES)
def test_mis_with_emission_and_area_hazards(pkg, api, orc, contexts, name):
    """The NEE twin's rigs, rays and assertions with rt_mis_trace against tests/mis_reference.py — records that hold an inf or a NaN
    included, under the NaN-position rule; on top the reverse map bit for bit, with RT_MIS_NO_ENTRY in the object record of an emitter
    the table's rules exclude as a whole (emission-inf, radius-0)."""
    bases, t0 = 0, time.perf_counter()
    for what, rig, planted, table, est, expect in _emission_and_area_hazards(pkg, api, orc, contexts, name, mr.Estimator, "radiance_trace_mis", "rt_mis_trace"):
        objects, words = _assert_map(pkg, api, what, rig)
        assert (objects[planted] == mr.NO_ENTRY) == (name in ("emission-inf", "radius-0")) == (not table["in_table"][planted]), what
        _not_vacuous(what, est, expect, t0)
        t0 = time.perf_counter()
        bases += 1
    assert bases >= 2


# ---- one context through hazards and back -----------------------------------------------------------------------------------------------

SEQUENCE = ("start", "sphere centre NaN", "sphere back", "matrix singular", "matrix back", "matrix NaN entry", "matrix back again")
SEQUENCE_TABLES = (1, 0, 1, 1, 1, 0, 1)   # a singular pair is finite: by rt_primary.h's rule the tables stay on (the root filter is what it drops)


def _sequence(pkg, lib, builder, tr, watch):
    rig = hz.Rig(pkg, builder, "flat-tables")
    t = rig.targets
    rig.upload(tr)
    tr.reset_counters()
    spheres, models = rig.spheres.copy(), rig.models.copy()
    l2w = hz._from_abi(models[t.model]["localToWorld"])
    frame, out = rig.frame0, []
    for step in SEQUENCE:
        s, m = spheres.copy(), models.copy()
        if step == "sphere centre NaN":
            s[t.sphere]["centre"][0] = np.nan
        if step in ("matrix singular", "matrix NaN entry"):
            m[t.model]["localToWorld"], m[t.model]["worldToLocal"] = hz.matrix_pair(l2w, "singular" if step == "matrix singular" else "nan")
        tr.update_spheres(s)
        tr.update_models(m)
        seen = []
        for n in (1, 2):   # a single frame, then a fused launch
            rig.p.frame = frame
            tr.set_params(rig.p)
            tr.render_frame() if n == 1 else tr.render_frames(n)
            frame += n
            img = tr.read_accumulated().copy()
            seen.append((img, tr.read_frame().copy(), tr.counters()["segments"], watch(tr)))
        out.append(seen)
    return out


def test_one_context_through_hazards_and_back(pkg, api, orc, contexts):
    """rt_update_spheres swaps a finite sphere for a NaN-centred one and back, rt_update_models a regular matrix pair for a singular one,
    for one with a NaN entry, and back; a single frame and a fused launch after each step.  The tables go off with the NaN and come back
    on, and every image equals the oracle's, which took the same steps."""
    ot = orc.create_tracer(8)
    try:
        want = _sequence(pkg, orc, orc, ot, lambda tr: None)
    finally:
        ot.close()
    for name, env, tr, stats in contexts:
        if name != "default":
            continue
        got = _sequence(pkg, api, api, tr, _tables)
        for step, expect_on, g, w in zip(SEQUENCE, SEQUENCE_TABLES, got, want):
            for part, (ga, gf, gs, gd), (wa, wf, ws, _) in zip(("single frame", "fused launch"), g, w):
                what = f"{step}, {part} ({'STATS' if stats else 'shipped'})"
                print(f"{what}: segments {gs} (oracle {ws}), tables {gd}")
                hz.assert_image(ga, wa, what + ": AccumulatedRender != oracle")
                hz.assert_image(gf, wf, what + ": FrameRender != oracle")
                assert gs == ws, what
                assert gd == ((1, 1, 1) if expect_on else (0, 0, 0)), f"{what}: rt_debug_primary_table / _tile_cand / _tile_tri = {gd}"
        if stats:
            assert tr.phase_profile()["filter_violations"][0] == 0


# ---- the triangle values ----------------------------------------------------------------------------------------------------------------

def _boundary_rays(rig, t):
    """rays from the camera origin and from 3 other origins to every corner, every edge midpoint and the centroid of the 16 most seen
    triangles: where tri_test's u, v, w >= 0 tests sit at 0.  The points are computed in fp32 from the uploaded records and taken to
    world space with the record's own localToWorld; in order, then reversed.  -> (origins, directions), fp32"""
    pts = []
    with np.errstate(all="ignore"):
        for mi, ti, _ in t.most_seen[:16]:
            T = rig.triangles[ti]
            a, b, c = (T[p].astype(F) for p in hz.POS)
            local = [a, b, c, (a + b) * F(0.5), (b + c) * F(0.5), (c + a) * F(0.5), (a + b + c) / F(3)]
            pts.append(hz._mul_point(rig.models["localToWorld"][mi], np.stack(local), 1))
        pts = np.concatenate(pts).astype(F)
        cam = np.array(list(rig.p.camLocalToWorld), dtype=F)[12:15]
        centre = pts.mean(axis=0, dtype=F)
        # beside and above the camera, and the camera mirrored through the middle of the points (their back faces)
        origins = [cam, cam + np.array([0.9, 0.4, 0.0], dtype=F), cam + np.array([-0.6, 0.8, 0.3], dtype=F), centre + (centre - cam)]
        o = np.concatenate([np.broadcast_to(q, pts.shape) for q in origins]).astype(F)
        d = np.concatenate([pts - q for q in origins]).astype(F)
        d = (d / np.sqrt((d * d).sum(axis=1, keepdims=True), dtype=F)).astype(F)
    o, d = np.concatenate([o, o[::-1]]), np.concatenate([d, d[::-1]])
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


@pytest.mark.parametrize("base", ("bvh", "many"))
@pytest.mark.parametrize("name", (None, "tri-coincident"), ids=("unplanted", "tri-coincident"))
def test_rays_at_the_corners_and_edges_of_the_most_seen_triangles(pkg, api, orc, contexts, base, name):
    """rt_query_closest and rt_debug_intersect on rays aimed at the boundaries of tri_test's >= 0 tests: every field == oracle_ray_collision,
    and (object, triangle) one the oracle's hit can be.  A ray through an edge two triangles share, and every hit on a coincident pair, is
    a tie that the walk order and the strict < decide: the normal and the backface bit say which of the two won."""
    abi = pkg.abi
    case = hz.BY_NAME[name] if name else None
    t = hz.aim(pkg, base)
    rig, tr, ot = _side_setup(pkg, api, orc, contexts, base, case)
    try:
        o, d = _boundary_rays(hz.Rig(pkg, api, base), t)   # aimed at the unplanted records: the coincident pairs keep every even triangle
        assert 800 <= len(o) <= 1200 and np.isfinite(o).all() and np.isfinite(d).all()
        hits10 = _oracle_hits(orc, ot, o, d)
        want, hit = _hit_records(abi, abi.RAYHIT_DTYPE, hits10)
        what = f"{name or 'unplanted'} on {base}, boundary rays"
        got = tr.query_closest(abi.make_rays(o, d))
        assert np.array_equal(got["object"] >= 0, hit), what + ": rt_query_closest: object >= 0 exactly where the oracle hits"
        _assert_fields(got, want, ("dst", "normal", "pos", "hit"), what + ": rt_query_closest")
        named, ties = _assert_named(pkg, orc, rig, o, d, hits10, got["object"], got["triangle"], what)
        dbg = tr.debug_intersect(o, d)
        ok = _same(dbg, hits10)
        ok[~hit, 3:] = True
        assert ok.all(), f"{what}: rt_debug_intersect: {int((~ok.all(axis=1)).sum())} rays differ from oracle_ray_collision"
        back = int((hits10[hit, 1] != 0).sum())
        print(f"{what}: {len(o)} rays, {int(hit.sum())} hit ({back} a back face), {named} named, {ties} ties")
        assert hit.sum() >= len(o) // 4 and named >= len(o) // 4 and (ties > 0 or name is None), what
    finally:
        ot.close()


@pytest.mark.parametrize("base", hz.BASES)
def test_determinant_exactly_at_the_threshold(pkg, api, orc, contexts, base):
    """tri_test keeps a triangle with `determinant >= 1E-8f`: a ray whose determinant is the float below 1E-8f, 1E-8f itself and the float
    above it (hazard_scenes.threshold_rig; tests/test_hazards.py holds the premises) through rt_query_closest, rt_debug_intersect and
    rt_query_occluded == oracle_ray_collision: a miss of the planted triangle, a hit, a hit.  (`>` for `>=` differs at the middle one alone,
    and nowhere else in this suite.)"""
    abi = pkg.abi
    tr = next(t for name, _, t, stats in contexts if name == "default" and not stats)
    for which, (s1, s2) in hz.threshold_edges().items():
        rig, o, d = hz.threshold_rig(pkg, api, base, s1, s2)
        rig.upload(tr)
        ot = orc.create_tracer(1)
        try:
            hz.threshold_rig(pkg, orc, base, s1, s2)[0].upload(ot)
            hits10 = _oracle_hits(orc, ot, o, d)
        finally:
            ot.close()
        want, hit = _hit_records(abi, abi.RAYHIT_DTYPE, hits10)
        what = f"determinant {which} 1E-8f on {base}"
        near = bool(hit[0]) and abs(float(hits10[0, 2]) - 0.01) < 1e-4
        assert near == (which != "below"), what
        got = tr.query_closest(abi.make_rays(o, d))
        assert np.array_equal(got["object"] >= 0, hit), what
        _assert_fields(got, want, ("dst", "normal", "pos", "hit"), what + ": rt_query_closest")
        if near:
            lo = int(rig.models["triOffset"][0])
            assert int(got["object"][0]) >= rig.n_spheres and lo <= int(got["triangle"][0]) < lo + int(rig.tri_count[0]), what
        dbg = tr.debug_intersect(o, d)
        ok = _same(dbg, hits10)
        ok[~hit, 3:] = True
        assert ok.all(), what + ": rt_debug_intersect"
        occ = tr.query_occluded(abi.make_rays(o, d, np.full(1, 0.02, dtype=F)))
        assert int(occ[0]) == int(bool(hit[0]) and hits10[0, 2] < F(0.02)) == int(near), what + ": rt_query_occluded within 0.02"
        print(f"{what}: hit {bool(hit[0])} at {hits10[0, 2]}")


@pytest.mark.parametrize("base", hz.LAYOUT_BASES)
@pytest.mark.parametrize("name", hz.LAYOUT_CASES)
def test_triangle_values_under_the_layout_that_moves_the_records(pkg, api, orc, name, base):
    """RT_LAYOUT=pre,arena,cache (read by rt_upload_scene): the triangle records are pre-differenced and moved into the arena; the same
    frames, counters and audit as under the default layout"""
    layout = "pre,arena,cache"
    case = hz.BY_NAME[name]
    rig = hz.Rig(pkg, api, base, case)
    used = api.layout_arrays(rig.models, rig.triangles, rig.nodes, layout)["used"]
    assert "pre" in used.split(",") and "arena" in used.split(","), f"asked for {layout}, the scene is laid out as {used}"
    with environment({"RT_LAYOUT": layout}, ENV):
        for stats in (False, True):
            tr = api.create_tracer(0)
            try:
                tr.enable_stats(stats)
                _check(pkg, api, orc, case, base, "RT_LAYOUT=" + layout, {"RT_LAYOUT": layout}, tr, stats)
            finally:
                tr.close()


def _emissive(case, name):
    """the case with its triangle model made an opaque emitter"""
    def scene(pkg_, sc, t_):
        if case.scene:
            case.scene(pkg_, sc, t_)
        m = sc.models[t_.tri_model].material = copy.deepcopy(sc.models[t_.tri_model].material)
        m.flag, m.emissionCol, m.emissionStrength = 0, (1.0, 0.9, 0.7, 1.0), 5.0
    return hz.Case(name + "-emitter", case.kind, case.guard, case.tables, scene=scene, triangles=case.triangles)


def _planted_triangle_emitters(pkg, api, orc, contexts, name, estimator, trace, call, bases=hz.SIDE_BASES):
    """The body of the NEE test below, for either light-sampling pass (as _emission_and_area_hazards).  Yields per base
    (what, rig, the emissive model's object index, its triangle range, the planted triangles, the estimator, the expected records)"""
    abi = pkg.abi
    for base in bases:
        t = hz.aim(pkg, base)
        rig = hz.Rig(pkg, api, base, _emissive(hz.BY_NAME[name], name))
        tr = next(x for n, _, x, stats in contexts if n == "default" and not stats)
        rig.upload(tr)
        what = f"{name} on {base}"
        want = nr.light_table(abi, rig.models, rig.triangles, rig.spheres)
        got = api.light_table_arrays(rig.models, rig.triangles, rig.spheres)
        assert got["entries"].tobytes() == want["entries"].tobytes() and got["cdf"].tobytes() == want["cdf"].tobytes(), what
        counts = (want["n_sphere_entries"], want["n_triangle_entries"])
        assert (got["n_sphere_entries"], got["n_triangle_entries"]) == counts and tr.nee_light_count() == counts, what
        # which triangles of the emissive model are entries: its range without the planted ones
        obj = rig.n_spheres + t.tri_model
        lo = int(rig.models["triOffset"][t.tri_model])
        mine = set(range(lo, lo + int(rig.tri_count[t.tri_model])))
        planted = mine if name in ("tri-degenerate", "tri-tiny-1e-20") else {t.seen}
        listed = set(int(k) for k in want["entries"]["triangle"][want["entries"]["object"] == obj])
        assert listed == mine - planted, f"{what}: entries of the emissive model {sorted(listed)}, planted {sorted(planted)}"
        assert want["in_table"][obj] == bool(mine - planted), what
        assert np.isfinite(want["cdf"]).all() and np.isfinite(want["entries"]["prob"]).all() and np.isfinite(want["entries"]["ng"]).all()
        rig.p.numRaysPerPixel = 1
        p = rig.params(1)
        tr.set_params(p)
        o, d, state = rr.camera_rays(orc, p, rig.w, rig.h, frame=rig.frame0 + 1)
        rays = abi.make_path_rays(o.reshape(-1, 3), d.reshape(-1, 3), state.ravel())[::7]
        est = estimator(pkg, orc, tr, rig.models, rig.triangles, rig.spheres, p)
        expect = est.trace(rays)
        out = getattr(tr, trace)(rays)
        ok = _same(out["rgb"], expect["rgb"]).all(axis=1) & (out["rng"] == expect["rng"])
        print(f"{what}: lights {counts}, {len(listed)} of {len(mine)} triangles of the emissive model listed, {est.samples} samples, "
              f"{est.shadow_rays} shadow rays, {est.unshadowed} unshadowed")
        assert ok.all(), f"{what}: {call}: {int((~ok).sum())} of {len(ok)} rays differ from the restated estimator"
        yield what, rig, obj, (lo, lo + int(rig.tri_count[t.tri_model])), planted, est, expect


@pytest.mark.parametrize("name", hz.NEE_TRI_CASES)
def test_nee_with_an_emissive_model_of_planted_triangles(pkg, api, orc, contexts, name):
    """the light table's area rule (rt_light_table.h: S > 0 and finite, ng finite) on planted triangles: rt_debug_light_table == the numpy
    table of tests/nee_reference.py bit for bit, rt_nee_light_count, the planted triangles left out exactly where their area (float64
    from the fp32 world corners, rounded to fp32) is 0 or not finite; rt_nee_trace on every 7th pixel's camera ray == the restated estimator"""
    assert len(list(_planted_triangle_emitters(pkg, api, orc, contexts, name, nr.Estimator, "radiance_trace_nee", "rt_nee_trace"))) == len(hz.SIDE_BASES)


@pytest.mark.parametrize("name", hz.NEE_TRI_CASES)
def test_mis_with_an_emissive_model_of_planted_triangles(pkg, api, orc, contexts, name):
    """The NEE twin's rigs, rays and assertions with rt_mis_trace against tests/mis_reference.py; on top the reverse map bit for bit: a
    planted triangle the area rule leaves out has the word RT_MIS_NO_ENTRY INSIDE the range of a model whose object record has a base
    (a hole in the middle of the range: a hit there is added in full, the triangles around it are weighted), and a model all of whose
    triangles are left out has RT_MIS_NO_ENTRY in its object record and no words."""
    # tri-degenerate and tri-tiny-1e-20 plant every triangle of the emissive model's mesh, and on the bvh base that mesh is the cube the
    # room's light shares: the table is empty there, and an empty table is rt_radiance_trace (tests/test_gpu_mis.py holds that identity)
    # — no sample would be taken.  Those two cases take flat-tables, whose emissive spheres stay, in its place.
    whole_mesh = name in ("tri-degenerate", "tri-tiny-1e-20")
    bases = tuple("flat-tables" if (b == "bvh" and whole_mesh) else b for b in hz.SIDE_BASES)
    holes, t0 = 0, time.perf_counter()
    for what, rig, obj, (lo, hi), planted, est, expect in _planted_triangle_emitters(pkg, api, orc, contexts, name, mr.Estimator, "radiance_trace_mis", "rt_mis_trace", bases):
        objects, words = _assert_map(pkg, api, what, rig)
        whole = planted == set(range(lo, hi))
        assert (objects[obj] == mr.NO_ENTRY) == whole, what
        if not whole:
            base = int(objects[obj])
            assert base + (hi - lo) <= len(words), what
            for k in range(lo, hi):
                assert (words[base + (k - lo)] == mr.NO_ENTRY) == (k in planted), f"{what}: triangle {k} of the emissive model"
            holes += len(planted)
        _not_vacuous(what, est, expect, t0)
        t0 = time.perf_counter()
    assert (holes > 0) == (name in ("tri-vertex-1e20", "tri-vertex-nan")), f"{name}: {holes} words without an entry inside a range that has a base"


MESH = [c for c in hz.CASES if c.kind == "mesh"]


@pytest.mark.parametrize("case", MESH, ids=[c.name for c in MESH])
def test_gpu_builder_on_every_mesh_case(pkg, api, orc, case):
    """every planted mesh, with the other meshes of its base, through rt_build_bvh_gpu_batch: the host builder's bytes where it builds,
    its refusal (RT_ERR_SCENE) where it refuses; then a plain mesh again — the device and the builder's scratch pool stay usable"""
    plain = pkg.meshes.cube()
    host_plain = api.build_bvh_arrays(plain.vertices, plain.normals, plain.triangles)
    for base in hz.BASES:
        rig = hz.Rig(pkg, api, base, case)   # (the host builder)
        uniq = []
        for m in rig.meshes:
            if not any(m is u for u in uniq):
                uniq.append(m)
        try:
            nd, trs, per = api.build_bvh_arrays_gpu_batch([(m.vertices, m.normals, m.triangles) for m in uniq], rig.bvh_quality)
            outcome = None
        except pkg.abi.RtError as e:
            outcome = ("build_bvh", e.status)
        print(f"{case.name} on {base}: {len(uniq)} meshes, host {rig.refused or 'builds'}, device {outcome or 'builds'}")
        assert outcome == rig.refused and (rig.refused is None) == case.builds(base), (case.name, base, outcome, rig.refused)
        if outcome is None:
            assert nd.tobytes() == rig.nodes.tobytes() and trs.tobytes() == hz.Rig(pkg, orc, base, case).triangles.tobytes(), (case.name, base)
            assert trs.tobytes() == rig.triangles.tobytes()
        nd, trs, per = api.build_bvh_arrays_gpu_batch([(plain.vertices, plain.normals, plain.triangles)])
        assert nd.tobytes() == host_plain[0].tobytes() and trs.tobytes() == host_plain[1].tobytes(), (case.name, base, "a plain mesh afterwards")
    api.build_bvh_gpu_release()
