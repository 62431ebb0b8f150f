"""include/rt_nee.h without a GPU: the header is plain C (C99 and C++17) and RtLightEntry is 80 bytes with the documented offsets, which
abi.LIGHT_ENTRY_DTYPE matches field by field; hip.NEE_SYMBOLS is the header's list, disjoint from every other list, and the library
exports exactly it; the context calls refuse a null context; rt_debug_light_table (host only) gives the table
tests/nee_reference.py computes on its own in numpy; and ray-tracing_amd/csrc/rt_light_table.h with rt_nee_launch.h — the HIP-free half
of the feature — passes its stand-alone driver (tests/light_table_driver.cpp) built with the address and undefined-behaviour
sanitizers."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import host_driver

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nee_reference as nr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
ENTRY_OFFSETS = {"a": (0, 12), "size": (12, 4), "e1": (16, 12), "prob": (28, 4), "e2": (32, 12), "object": (44, 4), "ng": (48, 12), "triangle": (60, 4),
                 "emission": (64, 12), "reserved": (76, 4)}
FUNCTIONS = sorted(["rt_nee_trace", "rt_nee_trace_buffers", "rt_nee_light_count", "rt_debug_light_table", "rt_debug_light_table_free"])


def header_functions():
    text = open(os.path.join(INCLUDE, "rt_nee.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rt_[a-z_0-9]+)\s*\(", text)))


@pytest.mark.parametrize("lang", ["c99", "c++17"])
def test_header_compiles_and_has_the_documented_layout(lang, tmp_path):
    cxx = lang.startswith("c++")
    src = tmp_path / ("nee.cpp" if cxx else "nee.c")
    checks = "\n".join(f"typedef char entry_at_{f}[offsetof(RtLightEntry, {f}) == {o} && sizeof(((RtLightEntry*)0)->{f}) == {s} ? 1 : -1];" for f, (o, s) in ENTRY_OFFSETS.items())
    src.write_text('#include <stddef.h>\n#include "rt_nee.h"\ntypedef char entry_is_80[sizeof(RtLightEntry) == 80 ? 1 : -1];\n'
                   "typedef char cap_is_2_22[RT_NEE_MAX_LIGHTS == 4194304 ? 1 : -1];\n" + checks +
                   "\nint use(RtContext* c, RtPathRay* r, RtRadiance* o, RtLightTableDump* d) { int a = 0, b = 0; rt_debug_light_table_free(d);"
                   " return rt_nee_trace(c, r, 1, o) + rt_nee_trace_buffers(c, r, 1, o) + rt_nee_light_count(c, &a, &b)"
                   " + rt_debug_light_table(0, 0, 0, 0, 0, 0, d); }\n")
    cmd = ["g++", "-x", "c++"] if cxx else ["gcc", "-x", "c"]
    subprocess.check_call(cmd + [f"-std={lang}", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(src)])


def test_numpy_dtype_matches_the_header_field_by_field(pkg):
    abi = pkg.abi
    dtype = abi.LIGHT_ENTRY_DTYPE
    assert dtype.itemsize == 80 and dtype.names == tuple(ENTRY_OFFSETS) and abi.NEE_MAX_LIGHTS == 1 << 22
    for f, (off, nbytes) in ENTRY_OFFSETS.items():
        assert dtype.fields[f][1] == off and dtype.fields[f][0].itemsize == nbytes, f
    text = open(os.path.join(INCLUDE, "rt_nee.h")).read()
    body = re.search(r"typedef struct RtLightEntry \{(.*?)\} RtLightEntry;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = re.findall(r"(float|uint32_t|int32_t)\s+([a-z0-9]+)(?:\[(\d+)\])?;", body)
    kinds = {"float": "f", "uint32_t": "u", "int32_t": "i"}
    assert [d[1] for d in decl] == list(dtype.names)
    for ctype, name, count in decl:
        sub = dtype.fields[name][0]
        assert sub.base.kind == kinds[ctype] and sub.base.itemsize == 4 and sub.shape == ((int(count),) if count else ()), name


def test_header_symbols_are_exported_and_listed(pkg, api):
    names = header_functions()
    assert names == FUNCTIONS
    assert sorted(pkg.hip.NEE_SYMBOLS) == names, "hip.NEE_SYMBOLS is out of sync with include/rt_nee.h"
    for other in (pkg.hip.ABI_SYMBOLS, pkg.hip.COST_SYMBOLS, pkg.hip.PRIMARY_SYMBOLS, pkg.hip.TILE_CAND_SYMBOLS, pkg.hip.TILE_TRI_SYMBOLS, pkg.hip.AOV_SYMBOLS,
                  pkg.hip.DENOISE_SYMBOLS, pkg.hip.REPROJECT_SYMBOLS, pkg.hip.MOTION_SYMBOLS, pkg.hip.VARIANCE_SYMBOLS, pkg.hip.ADAPTIVE_SYMBOLS,
                  pkg.hip.QUERY_SYMBOLS, pkg.hip.RADIANCE_SYMBOLS):
        assert not set(names) & set(other)
    for n in names:
        assert hasattr(api.lib, n), f"libraytrace_hip.so does not export {n}"
    exported = subprocess.run(["nm", "-D", "--defined-only", api.lib._name], capture_output=True, text=True, check=True).stdout
    mine = sorted(set(re.findall(r"\b(rt_[a-z_0-9]*(?:nee|light_table)[a-z_0-9]*)\b", exported)))
    assert mine == names, "the library exports a call of this family that the header does not declare"


def test_every_context_call_refuses_a_null_context(pkg, api):
    import ctypes as C
    rays = pkg.abi.make_path_rays([[0, 0, 0]], [[0, 0, 1]], 1)
    out = np.zeros(1, dtype=pkg.abi.RADIANCE_DTYPE)
    for call in (api.nee_trace, api.nee_trace_buffers):
        assert call(None, rays.ctypes.data, 1, out.ctypes.data) == pkg.abi.RT_ERR_INVALID_ARG
        assert b"null context" in api.last_error(None)
        assert call(None, None, 0, None) == pkg.abi.RT_ERR_INVALID_ARG
    a, b = C.c_int(7), C.c_int(7)
    assert api.nee_light_count(None, C.byref(a), C.byref(b)) == pkg.abi.RT_ERR_INVALID_ARG and (a.value, b.value) == (7, 7)
    assert not out.view(np.uint32).any()


def test_debug_light_table_needs_no_device_and_matches_the_numpy_table(pkg, api):
    """The library's table (rt_light_table.h, C++) against tests/nee_reference.py's (numpy float64 rounded to float32, written from the
    header text): every field of every entry and the cdf, as bits.  The scene has every kind of exclusion, a mirrored instance and
    unevenly sized emitters."""
    import ctypes as C
    abi = pkg.abi
    models, tris, spheres = nr.table_test_scene(abi)
    got = api.light_table_arrays(models, tris, spheres)
    want = nr.light_table(abi, models, tris, spheres)
    assert got["n_sphere_entries"] == want["n_sphere_entries"] == 3 and got["n_triangle_entries"] == want["n_triangle_entries"] == 6
    assert got["entries"].tobytes() == want["entries"].tobytes()
    assert got["cdf"].tobytes() == want["cdf"].tobytes() and got["cdf"][-1] == 1.0 and (np.diff(got["cdf"]) >= 0).all()
    for u in [0.0, 1.0] + [float(c) for c in got["cdf"]] + [float(np.nextafter(c, np.float32(0))) for c in got["cdf"]]:
        below = np.nonzero(np.float32(u) < got["cdf"])[0]
        assert nr.pick(got["cdf"], np.float32(u)) == (below[0] if len(below) else len(got["cdf"]) - 1)
    # no scene at all; the error rows
    empty = api.light_table_arrays(None, None, None)
    assert len(empty["entries"]) == 0 and len(empty["cdf"]) == 0
    d = abi.RtLightTableDump()
    assert api.debug_light_table(None, 0, None, 0, None, 0, None) == abi.RT_ERR_INVALID_ARG
    assert api.debug_light_table(None, 1, None, 0, None, 0, C.byref(d)) == abi.RT_ERR_INVALID_ARG and b"rt_debug_light_table" in api.last_error(None)
    assert api.debug_light_table(None, 0, None, -1, None, 0, C.byref(d)) == abi.RT_ERR_INVALID_ARG
    bad = models.copy()
    bad["triOffset"][0] = len(tris) + 1
    assert api.debug_light_table(bad.ctypes.data, len(bad), tris.ctypes.data, len(tris), None, 0, C.byref(d)) == abi.RT_ERR_INVALID_ARG
    assert not d.entries and not d.cdf
    api.debug_light_table_free(C.byref(d))


def test_light_table_driver_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    """Which objects become entries (glass, NaN, non-positive, zero-area, zero-radius, checkered), the mirrored transform's swap, one set
    of entries per instance, the cdf and the pick rule at 0, 1 and every cdf value, the entry cap, the dump, and rt_nee_launch.h's
    argument checks and sizes.  A program of its own: nothing of it is loaded into this process."""
    exe = host_driver.build(tmp_path, "light_table", ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
                            exe="light_table_driver")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "LIGHT_TABLE_OK", (p.returncode, p.stdout, p.stderr)
