"""include/rt_mis.h without a GPU: the header is plain C (C99 and C++17) and RtMisBatch is 40 bytes with the documented offsets, which
abi.MisBatch matches field by field; hip.MIS_SYMBOLS is the header's list, disjoint from every other list, and the library exports
exactly it; rt_mis_trace refuses a descriptor that is not this library's before it reads or writes anything; rt_debug_light_map (host
only) gives the map tests/mis_reference.py computes on its own from the numpy table; and ray-tracing_amd/csrc/rt_light_table.h's
build_map with rt_mis_launch.h — the HIP-free half of the feature — passes its stand-alone driver (tests/mis_map_driver.cpp) built with
the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import host_driver

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mis_reference as mr  # noqa: E402
import nee_reference as nr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
BATCH_OFFSETS = {"struct_size": (0, 4), "memory": (4, 4), "ctx": (8, 8), "rays": (16, 8), "out": (24, 8), "n": (32, 4), "reserved": (36, 4)}
FUNCTIONS = sorted(["rt_mis_trace", "rt_debug_light_map", "rt_debug_light_map_free"])


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "rt_mis.h")).read(), flags=re.S)


@pytest.mark.parametrize("lang", ["c99", "c++17"])
def test_header_compiles_and_has_the_documented_layout(lang, tmp_path):
    cxx = lang.startswith("c++")
    src = tmp_path / ("mis.cpp" if cxx else "mis.c")
    checks = "\n".join(f"typedef char batch_at_{f}[offsetof(RtMisBatch, {f}) == {o} && sizeof(((RtMisBatch*)0)->{f}) == {s} ? 1 : -1];" for f, (o, s) in BATCH_OFFSETS.items())
    src.write_text('#include <stddef.h>\n#include "rt_mis.h"\ntypedef char batch_is_40[sizeof(RtMisBatch) == 40 ? 1 : -1];\n'
                   "typedef char forms[RT_MIS_HOST == 0 && RT_MIS_DEVICE == 1 && RT_MIS_NO_ENTRY == 0xffffffffu ? 1 : -1];\n" + checks +
                   "\nint use(RtMisBatch* b, RtLightMapDump* d) { rt_debug_light_map_free(d); return rt_mis_trace(b) + rt_debug_light_map(0, 0, 0, 0, 0, 0, d); }\n")
    cmd = ["g++", "-x", "c++"] if cxx else ["gcc", "-x", "c"]
    subprocess.check_call(cmd + [f"-std={lang}", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(src)])


def test_ctypes_mirror_matches_the_header_field_by_field(pkg):
    abi = pkg.abi
    assert C.sizeof(abi.MisBatch) == 40 and [f[0] for f in abi.MisBatch._fields_] == list(BATCH_OFFSETS)
    for f, (off, nbytes) in BATCH_OFFSETS.items():
        d = getattr(abi.MisBatch, f)
        assert (d.offset, d.size) == (off, nbytes), f
    body = re.search(r"typedef struct RtMisBatch \{(.*?)\} RtMisBatch;", header_text(), flags=re.S).group(1)
    decl = re.findall(r"(uint32_t|int32_t|RtContext\s*\*|const void\s*\*|void\s*\*)\s*([a-z_]+);", body)
    assert [d[1] for d in decl] == list(BATCH_OFFSETS)
    kinds = {"uint32_t": C.c_uint32, "int32_t": C.c_int32}
    for (ctype, name), (fname, ftype) in zip(decl, abi.MisBatch._fields_):
        assert ftype is kinds.get(ctype, C.c_void_p), name
    assert (abi.MIS_HOST, abi.MIS_DEVICE, abi.MIS_NO_ENTRY) == (0, 1, 0xFFFFFFFF)
    dump = re.search(r"typedef struct RtLightMapDump \{(.*?)\} RtLightMapDump;", header_text(), flags=re.S).group(1)
    assert re.findall(r"\b([a-z_]+)\s*[;,]", dump) == [f[0] for f in abi.RtLightMapDump._fields_]
    assert C.sizeof(abi.RtLightMapDump) == 32


def test_header_symbols_are_exported_and_listed(pkg, api):
    names = sorted(set(re.findall(r"\b(rt_[a-z_0-9]+)\s*\(", header_text())))
    assert names == FUNCTIONS
    assert sorted(pkg.hip.MIS_SYMBOLS) == names, "hip.MIS_SYMBOLS is out of sync with include/rt_mis.h"
    others = [getattr(pkg.hip, k) for k in dir(pkg.hip) if k.endswith("_SYMBOLS") and k != "MIS_SYMBOLS"]
    assert len(others) >= 15
    for other in others:
        assert not set(names) & set(other)
    for n in names:
        assert hasattr(api.lib, n), f"libraytrace_hip.so does not export {n}"
    exported = subprocess.run(["nm", "-D", "--defined-only", api.lib._name], capture_output=True, text=True, check=True).stdout
    mine = sorted(set(re.findall(r"\b(rt_mis_[a-z_0-9]*|rt_debug_light_map[a-z_0-9]*)\b", exported)))
    assert mine == names, "the library exports a call of this family that the header does not declare"


def test_a_descriptor_that_is_not_this_librarys_is_refused_and_nothing_is_written(pkg, api):
    abi = pkg.abi
    rays = abi.make_path_rays([[0, 0, 0]], [[0, 0, 1]], 1)
    out = np.zeros(1, dtype=abi.RADIANCE_DTYPE)
    fake_ctx = (C.c_char * 4096)()  # never read: every row below is refused before the context is looked at

    def batch(**kw):
        b = abi.MisBatch()
        b.struct_size, b.memory, b.ctx, b.rays, b.out, b.n, b.reserved = 40, abi.MIS_HOST, C.addressof(fake_ctx), rays.ctypes.data, out.ctypes.data, 1, 0
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    assert api.mis_trace(None) == abi.RT_ERR_INVALID_ARG and b"null descriptor" in api.last_error(None)
    for what, b, text in (("a null ctx", batch(ctx=None), b"null context"),
                          ("struct_size 36", batch(struct_size=36), b"struct_size"),
                          ("struct_size 0", batch(struct_size=0), b"struct_size"),
                          ("struct_size 48", batch(struct_size=48), b"struct_size"),
                          ("reserved 1", batch(reserved=1, ctx=None), b"reserved"),
                          ("reserved -1", batch(reserved=-1, ctx=None), b"reserved"),
                          ("memory 2", batch(memory=2, ctx=None), b"memory"),
                          ("memory 2^32 - 1", batch(memory=0xFFFFFFFF, ctx=None), b"memory")):  # (with a context: tests/test_gpu_mis.py)
        assert api.mis_trace(C.byref(b)) == abi.RT_ERR_INVALID_ARG, what
        assert text in api.last_error(None), (what, api.last_error(None))
    assert not out.view(np.uint32).any() and not bytes(fake_ctx).strip(b"\0")


def test_debug_light_map_needs_no_device_and_matches_the_numpy_map(pkg, api):
    """The library's map (rt_light_table.h build_map, C++) against tests/mis_reference.py's, made from tests/nee_reference.py's numpy
    table: word for word, and every (object, triangle) of the scene maps to the entry whose fields say so, or to none.  The scene holds
    every exclusion rule, a mirrored instance and an instanced mesh."""
    abi = pkg.abi
    models, tris, spheres = nr.table_test_scene(abi)
    got = api.light_map_arrays(models, tris, spheres)
    objects, words, table = mr.map_arrays(abi, models, tris, spheres)
    assert got["n_entries"] == len(table["entries"]) == 9
    assert np.array_equal(got["objects"], objects) and np.array_equal(got["triangles"], words)
    entries = table["entries"]
    n_sph = len(spheres)
    offsets = sorted(int(o) for o in models["triOffset"])
    reached = set()
    for o in range(n_sph + len(models)):
        if o < n_sph:
            keys = [-1]
        else:
            start = int(models[o - n_sph]["triOffset"])
            keys = range(start, min([x for x in offsets if x > start], default=len(tris)))
        for k in keys:
            base = int(got["objects"][o])
            e = base if (o < n_sph or base == abi.MIS_NO_ENTRY) else int(got["triangles"][base + k - int(models[o - n_sph]["triOffset"])])
            want = [i for i in range(len(entries)) if int(entries[i]["object"]) == o and int(entries[i]["triangle"]) == k]
            assert len(want) <= 1
            assert e == (want[0] if want else abi.MIS_NO_ENTRY), (o, k)
            reached.update(want)
    assert reached == set(range(len(entries)))
    # what the scene is there for: excluded spheres, a dark model, a glass model, a zero-area triangle and two models on one mesh
    assert (got["objects"][:n_sph] == abi.MIS_NO_ENTRY).sum() == 5 and (got["objects"][n_sph:] == abi.MIS_NO_ENTRY).sum() == 2
    assert (got["triangles"] == abi.MIS_NO_ENTRY).sum() == 1 and models["triOffset"][0] == models["triOffset"][2]
    # no scene at all; the error rows
    empty = api.light_map_arrays(None, None, None)
    assert len(empty["objects"]) == 0 and len(empty["triangles"]) == 0 and empty["n_entries"] == 0
    d = abi.RtLightMapDump()
    assert api.debug_light_map(None, 0, None, 0, None, 0, None) == abi.RT_ERR_INVALID_ARG
    assert api.debug_light_map(None, 1, None, 0, None, 0, C.byref(d)) == abi.RT_ERR_INVALID_ARG and b"rt_debug_light_map" in api.last_error(None)
    bad = models.copy()
    bad["triOffset"][0] = len(tris) + 1
    assert api.debug_light_map(bad.ctypes.data, len(bad), tris.ctypes.data, len(tris), None, 0, C.byref(d)) == abi.RT_ERR_INVALID_ARG
    assert not d.objects and not d.triangles
    api.debug_light_map_free(C.byref(d))


def test_the_far_emitter_is_an_entry_that_is_neither_sampled_nor_hit(pkg, api, orc):
    """The scene meant to give weights of exactly 0: tests/hazard_scenes.py's bvh base (config 3's room without its back wall) with an
    emissive sphere of radius 1e19 centred 3e19 behind the missing wall.  r2 = 1e38 is finite, d2 = 9e38 overflows to inf, so s2 = q = 0,
    pl' = inf and, by the header's rule, wb = pb / (pb + inf) = 0 for a lobe ray that reaches it — but nothing does, and no sample is
    ever taken either, so no GPU case is built on it:
      * the table takes the sphere (the library's and the numpy one), with prob = 1 to fp32: its power dwarfs the room's light;
      * the sampler: z = normalize(w) = w * rsqrt(inf) = 0, ct = 1, st = 0, so omega = 0 and cn = dot(n, 0) = 0: "nothing is added";
      * the intersection: c = dot(offset, offset) - r2 = inf, discriminant = b * b - 4 * a * c = inf - inf = NaN: a miss, for every ray.
    Held here without a GPU, from the oracle's RaySphere and the reference's sampler, so that a change of either is noticed."""
    import ctypes
    import hazard_scenes as hz

    def scene(pkg_, sc, t_):
        M = pkg_.RayTracingMaterial
        sc.spheres.append(pkg_.Sphere((0.0, 2.0, 3e19), 1e19, M(diffuseCol=(0, 0, 0, 1), emissionCol=(1, 0.9, 0.7, 1), emissionStrength=5.0)))
    rig = hz.Rig(pkg, orc, "bvh", hz.Case("far-emitter", "model", "shade", "on", scene=scene))
    assert len(rig.spheres) == 1 and rig.spheres["radius"][0] == np.float32(1e19)
    est = mr.Estimator(pkg, orc, None, rig.models, rig.triangles, rig.spheres, rig.params(1))
    table = est.table
    got = api.light_table_arrays(rig.models, rig.triangles, rig.spheres)
    assert got["entries"].tobytes() == table["entries"].tobytes() and got["cdf"].tobytes() == table["cdf"].tobytes()
    assert table["in_table"][0] and table["n_sphere_entries"] == 1 and table["entries"][0]["size"] == np.float32(1e38) and table["entries"][0]["prob"] == 1.0
    assert api.light_map_arrays(rig.models, rig.triangles, rig.spheres)["objects"][0] == 0
    x, n = np.array([0.3, 1.0, 1.0], dtype=np.float32), np.array([0, 0, 1], dtype=np.float32)
    with np.errstate(all="ignore"):
        for state in range(1, 33):
            assert est.sample(ctypes.c_uint32(state), x, n) is None
        assert est.samples == 32 and est.triangle_samples == 0 and est.inside == 0, "every draw picks the sphere, is outside it, and is rejected at cn > 0"
        wb, rule = est.emission_weight(0, -1, False, np.float32(0.5), x, n, np.array([0, 0, 2e19], dtype=np.float32))
        assert (float(wb), rule) == (0.0, mr.WEIGHTED), "the weight a hit would get"
    ot = orc.create_tracer(1)
    try:
        rig.upload(ot)
        F3, out = ctypes.c_float * 3, (ctypes.c_float * 10)()
        for d in ((0, 0, 1), (0.01, 0.02, 1), (0.2, 0.1, 1), (-0.3, 0.05, 1)):
            d = np.array(d, dtype=np.float64) / np.linalg.norm(d)
            orc.ray_collision(ot.h, F3(0.3, 1.0, 1.0), F3(*d), out)
            assert out[0] == 0.0, f"the ray along {d} hits {list(out)}"
    finally:
        ot.close()


def test_mis_map_driver_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    """The table and the map of generated scenes (instances, mirrored, dark and glass models, zero-area triangles, excluded spheres),
    the packed device words and the lookup for every hit and for triangles outside a model's range.  A program of its own: nothing
    of it is loaded into this process."""
    exe = host_driver.build(tmp_path, "mis_map", ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
                            exe="mis_map_driver")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "MIS_MAP_OK", (p.returncode, p.stdout, p.stderr)
