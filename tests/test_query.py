"""include/rt_query.h without a GPU: the header is plain C (C99 and C++17), RtRay is 32 and RtRayHit 48 bytes with the same field offsets
in C and in the numpy dtypes of abi.py; hip.QUERY_SYMBOLS is the header's list and the library exports it; each call refuses a null
context and what the header's error list names that needs no device; and ray-tracing_amd/csrc/rt_query_launch.h — the HIP-free half
of the entry points — passes its stand-alone driver (tests/query_launch_driver.cpp) built with the address and undefined-behaviour
sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest

import host_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
RAY_OFFSETS = {"origin": (0, 12), "tmax": (12, 4), "dir": (16, 12), "reserved": (28, 4)}
HIT_OFFSETS = {"dst": (0, 4), "normal": (4, 12), "pos": (16, 12), "hit": (28, 4), "object": (32, 4), "triangle": (36, 4), "reserved": (40, 8)}
FUNCTIONS = ["rt_query_closest", "rt_query_closest_buffers", "rt_query_occluded", "rt_query_occluded_buffers"]


def header_functions():
    text = open(os.path.join(INCLUDE, "rt_query.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rt_[a-z_0-9]+)\s*\(", text)))


@pytest.mark.parametrize("lang", ["c99", "c++17"])
def test_header_compiles_and_has_the_documented_layout(lang, tmp_path):
    cxx = lang.startswith("c++")
    src = tmp_path / ("query.cpp" if cxx else "query.c")
    checks = "\n".join(f"typedef char ray_at_{f}[offsetof(RtRay, {f}) == {o} && sizeof(((RtRay*)0)->{f}) == {s} ? 1 : -1];" for f, (o, s) in RAY_OFFSETS.items())
    checks += "\n" + "\n".join(f"typedef char hit_at_{f}[offsetof(RtRayHit, {f}) == {o} && sizeof(((RtRayHit*)0)->{f}) == {s} ? 1 : -1];"
                               for f, (o, s) in HIT_OFFSETS.items())
    src.write_text('#include <stddef.h>\n#include "rt_query.h"\ntypedef char ray_is_32[sizeof(RtRay) == 32 ? 1 : -1];\n'
                   "typedef char hit_is_48[sizeof(RtRayHit) == 48 ? 1 : -1];\ntypedef char max_is_2_26[RT_QUERY_MAX_RAYS == 67108864 ? 1 : -1];\n" + checks +
                   "\nint use(RtContext* c, RtRay* r, RtRayHit* h, uint32_t* o) { return rt_query_closest(c, r, 1, h) + rt_query_closest_buffers(c, r, 1, h)"
                   " + rt_query_occluded(c, r, 1, o) + rt_query_occluded_buffers(c, r, 1, o) + (int)(RT_AOV_HIT_BACKFACE | RT_AOV_HIT_GLASS); }\n")
    cmd = ["g++", "-x", "c++"] if cxx else ["gcc", "-x", "c"]
    subprocess.check_call(cmd + [f"-std={lang}", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(src)])


def test_numpy_dtypes_match_the_header_field_by_field(pkg):
    abi = pkg.abi
    for dtype, offsets, size in ((abi.RAY_DTYPE, RAY_OFFSETS, 32), (abi.RAYHIT_DTYPE, HIT_OFFSETS, 48)):
        assert dtype.itemsize == size and dtype.names == tuple(offsets)
        for f, (off, nbytes) in offsets.items():
            assert dtype.fields[f][1] == off and dtype.fields[f][0].itemsize == nbytes, f
    # the field types, as the header's declarations state them
    text = open(os.path.join(INCLUDE, "rt_query.h")).read()
    kinds = {"float": "f", "uint32_t": "u", "int32_t": "i"}
    for struct, dtype in (("RtRay", abi.RAY_DTYPE), ("RtRayHit", abi.RAYHIT_DTYPE)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        decl = re.findall(r"(float|uint32_t|int32_t)\s+([a-z]+)(?:\[(\d+)\])?;", body)
        assert [d[1] for d in decl] == list(dtype.names), struct
        for ctype, name, count in decl:
            sub = dtype.fields[name][0]
            assert sub.base.kind == kinds[ctype] and sub.base.itemsize == 4 and sub.shape == ((int(count),) if count else ()), (struct, name)
    assert abi.QUERY_MAX_RAYS == 1 << 26
    r = abi.make_rays([[1, 2, 3], [4, 5, 6]], [[0, 0, 1], [0, 1, 0]], tmax=[np.inf, 2.5])
    assert r.dtype == abi.RAY_DTYPE and r.tobytes() == np.array([1, 2, 3, np.inf, 0, 0, 1, 0, 4, 5, 6, 2.5, 0, 1, 0, 0], dtype=np.float32).tobytes()


def test_header_symbols_are_exported_and_listed(pkg, api):
    names = header_functions()
    assert names == FUNCTIONS
    assert sorted(pkg.hip.QUERY_SYMBOLS) == names, "hip.QUERY_SYMBOLS is out of sync with include/rt_query.h"
    for other in (pkg.hip.ABI_SYMBOLS, pkg.hip.COST_SYMBOLS, pkg.hip.AOV_SYMBOLS, pkg.hip.DENOISE_SYMBOLS, pkg.hip.REPROJECT_SYMBOLS, pkg.hip.MOTION_SYMBOLS,
                  pkg.hip.VARIANCE_SYMBOLS, pkg.hip.ADAPTIVE_SYMBOLS):
        assert not set(names) & set(other)
    for n in names:
        assert hasattr(api.lib, n), f"libraytrace_hip.so does not export {n}"
    exported = subprocess.run(["nm", "-D", "--defined-only", api.lib._name], capture_output=True, text=True, check=True).stdout
    mine = sorted(set(re.findall(r"\b(rt_query_[a-z_0-9]*)\b", exported)))
    assert mine == names, "the library exports a query call the header does not declare"


def test_every_call_refuses_a_null_context(pkg, api):
    rays = pkg.abi.make_rays([[0, 0, 0]], [[0, 0, 1]])
    out = np.zeros(16, dtype=np.uint32)
    for call in (api.query_closest, api.query_closest_buffers, api.query_occluded, api.query_occluded_buffers):
        assert call(None, rays.ctypes.data, 1, out.ctypes.data) == pkg.abi.RT_ERR_INVALID_ARG
        assert b"null context" in api.last_error(None)
        assert call(None, None, 0, None) == pkg.abi.RT_ERR_INVALID_ARG


def test_launch_header_driver_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    """Blocks and grid at n = 0, 1, 63, 64, 65, 2^26; the byte-size overflow guard; the overlap predicate on touching, nested and disjoint
    ranges; the shared argument checks.  A program of its own: nothing of it is loaded into this process."""
    exe = host_driver.build(tmp_path, "query_launch", ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
                            exe="query_launch_driver")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "QUERY_LAUNCH_OK", (p.returncode, p.stdout, p.stderr)
