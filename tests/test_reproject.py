"""rt_reproject / rt_resolve (include/rt_reproject.h) without a GPU: the header is plain C (C99 and C++17) and RtReprojectParams is the
same 100 bytes in C, in ctypes and through a numpy view; the library exports the header's six calls and each refuses a null context;
the default parameters are as the header states them; and the arithmetic of ray-tracing_amd/csrc/rt_reproject_math.h — the functions
the kernels call, here run by the host driver tests/reproject_math_driver.cpp — equals the NumPy restatement of the header's prose
(tests/reproject_reference.py) bit for bit, every pixel, every channel."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import host_driver
import reproject_reference as ref
from gpu_support import assert_same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
F = np.float32
OFFSETS = {"struct_size": 0, "prevViewParams": 4, "prevCamLocalToWorld": 16, "maxPlaneDistance": 80, "minNormalDot": 84, "maxHistory": 88, "flags": 92,
           "reserved": 96}
SIZES = {"prevViewParams": 12, "prevCamLocalToWorld": 64}
FUNCTIONS = ["rt_reproject_accumulated", "rt_reproject_buffers", "rt_reproject_default_params", "rt_resolve", "rt_resolve_buffers", "rt_resolve_to_device"]


def header_functions():
    text = open(os.path.join(INCLUDE, "rt_reproject.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rt_[a-z_0-9]+)\s*\(", text)))


# ---------------------------------------------------------------- 1. the header and the three layouts
@pytest.mark.parametrize("lang", ["c99", "c++17"])
def test_header_compiles_and_has_the_documented_layout(lang, tmp_path):
    cxx = lang.startswith("c++")
    src = tmp_path / ("rp.cpp" if cxx else "rp.c")
    checks = "\n".join(f"typedef char at_{f}[offsetof(RtReprojectParams, {f}) == {o} ? 1 : -1];" for f, o in OFFSETS.items())
    src.write_text('#include <stddef.h>\n#include "rt_reproject.h"\ntypedef char size_is_100[sizeof(RtReprojectParams) == 100 ? 1 : -1];\n' + checks +
                   "\nint use(RtContext* c, RtReprojectParams* p, float* f, RtPixelAov* a) { return rt_reproject_default_params(p)"
                   " + rt_reproject_buffers(c, p, 1, 1, f, a, a, f) + rt_reproject_accumulated(c, p, a, 1, a) + rt_resolve_buffers(c, 1, 1, f, f)"
                   " + rt_resolve(c, f, 16) + rt_resolve_to_device(c, f, 16) + (int)RT_REPROJECT_FLAG_GLASS; }\n")
    cmd = ["g++", "-x", "c++"] if cxx else ["gcc", "-x", "c"]
    subprocess.check_call(cmd + [f"-std={lang}", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(src)])


def test_ctypes_struct_and_numpy_view_are_the_same_100_bytes(pkg):
    abi = pkg.abi
    assert C.sizeof(abi.RtReprojectParams) == 100 and abi.REPROJECT_PARAMS_DTYPE.itemsize == 100
    assert tuple(n for n, _ in abi.RtReprojectParams._fields_) == tuple(OFFSETS) == abi.REPROJECT_PARAMS_DTYPE.names
    for f, off in OFFSETS.items():
        assert getattr(abi.RtReprojectParams, f).offset == off and getattr(abi.RtReprojectParams, f).size == SIZES.get(f, 4), f
        assert abi.REPROJECT_PARAMS_DTYPE.fields[f][1] == off, f
    p = abi.RtReprojectParams(struct_size=100, maxPlaneDistance=0.5, minNormalDot=0.25, maxHistory=64.0, flags=1, reserved=0)
    p.prevViewParams[:] = [1.0, 2.0, 3.0]
    p.prevCamLocalToWorld[:] = [float(i) for i in range(16)]
    a = np.frombuffer(bytes(p), dtype=abi.REPROJECT_PARAMS_DTYPE)[0]
    assert a["struct_size"] == 100 and a["prevViewParams"].tolist() == [1, 2, 3] and a["prevCamLocalToWorld"].tolist() == list(range(16))
    assert (a["maxPlaneDistance"], a["minNormalDot"], a["maxHistory"], a["flags"], a["reserved"]) == (0.5, 0.25, 64.0, 1, 0)
    assert struct.unpack("<I19f3fIi", bytes(p)) == (100, 1.0, 2.0, 3.0) + tuple(float(i) for i in range(16)) + (0.5, 0.25, 64.0, 1, 0)
    assert abi.REPROJECT_FLAG_GLASS == 1


# ---------------------------------------------------------------- 2. symbols  3. null context  4. default parameters
def test_header_symbols_are_exported_and_listed(pkg, api):
    names = header_functions()
    assert names == FUNCTIONS
    assert sorted(pkg.hip.REPROJECT_SYMBOLS) == names, "hip.REPROJECT_SYMBOLS is out of sync with include/rt_reproject.h"
    for other in (pkg.hip.ABI_SYMBOLS, pkg.hip.COST_SYMBOLS, pkg.hip.AOV_SYMBOLS, pkg.hip.DENOISE_SYMBOLS):
        assert not set(names) & set(other)
    for n in names:
        assert hasattr(api.lib, n), f"libraytrace_hip.so does not export {n}"


def test_every_call_refuses_a_null_context(pkg, api):
    abi = pkg.abi
    p = api.reproject_params()
    buf = np.zeros(64, dtype=np.float32)
    d = buf.ctypes.data
    assert api.reproject_buffers(None, C.byref(p), 1, 1, d, d, d, d) == abi.RT_ERR_INVALID_ARG
    assert b"null context" in api.last_error(None)
    assert api.reproject_accumulated(None, C.byref(p), d, 1, d) == abi.RT_ERR_INVALID_ARG
    assert api.reproject_accumulated(None, None, None, 1, None) == abi.RT_ERR_INVALID_ARG
    assert api.resolve_buffers(None, 1, 1, d, d) == abi.RT_ERR_INVALID_ARG
    assert api.resolve(None, d, 16) == abi.RT_ERR_INVALID_ARG
    assert api.resolve_to_device(None, d, 16) == abi.RT_ERR_INVALID_ARG
    assert api.reproject_default_params(None) == abi.RT_ERR_INVALID_ARG


def test_default_params_are_as_the_header_states_them(pkg, api):
    raw = (C.c_uint8 * 100)(*([0xff] * 100))
    p = pkg.abi.RtReprojectParams.from_buffer(raw)
    assert api.reproject_default_params(C.byref(p)) == pkg.abi.RT_OK
    assert p.struct_size == 100 and p.reserved == 0 and p.flags == 0
    assert list(p.prevViewParams) == [0.0] * 3 and list(p.prevCamLocalToWorld) == [0.0] * 16  # left for the caller
    assert (p.maxPlaneDistance, p.minNormalDot, p.maxHistory) == (F(0.1), F(0.9), 256.0)
    prev = pkg.abi.RtParams()
    prev.viewParams[:] = [2.0, 1.0, 3.0]
    prev.camLocalToWorld[:] = [float(i) for i in range(16)]
    q = api.reproject_params(prev, maxHistory=8.0, flags=1)
    assert list(q.prevViewParams) == [2.0, 1.0, 3.0] and list(q.prevCamLocalToWorld) == [float(i) for i in range(16)]
    assert (q.maxHistory, q.flags, q.minNormalDot) == (8.0, 1, p.minNormalDot)
    assert list(api.reproject_params(prevViewParams=(1, 2, 3)).prevViewParams) == [1.0, 2.0, 3.0]
    with pytest.raises(TypeError):
        api.reproject_params(maxDistance=1.0)


# ---------------------------------------------------------------- 5. the math header, through the host driver, against NumPy
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = host_driver.build(tmp_path_factory.mktemp("reproject_math"), "reproject_math", ["-std=c++17", "-O2", "-fno-fast-math", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"])

    def run(blob, h, w, via_file=None):
        if via_file:
            with open(via_file, "wb") as f:
                f.write(blob)
            out = subprocess.run([exe, str(via_file)], capture_output=True, timeout=600, check=True).stdout
        else:
            out = subprocess.run([exe], input=blob, capture_output=True, timeout=600, check=True).stdout
        return np.frombuffer(out, dtype=np.float32).reshape(h, w, 4)

    def reproject(rgba, prev, cur, view_params, cam, max_plane, min_dot, max_history, flags=0, via_file=None):
        h, w = rgba.shape[:2]
        blob = struct.pack("<4i", 0, w, h, flags) + np.array(list(view_params) + list(cam) + [max_plane, min_dot, max_history], dtype=F).tobytes()
        return run(blob + rgba.tobytes() + prev.tobytes() + cur.tobytes(), h, w, via_file)

    def resolve(rgba):
        h, w = rgba.shape[:2]
        return run(struct.pack("<4i", 1, w, h, 0) + rgba.tobytes(), h, w)
    reproject.resolve = resolve
    return reproject


def test_the_synthetic_views_cover_what_they_are_there_for(pkg, orc):
    w, h = 61, 35
    rgba, prev, cur, cam = ref.synthetic(pkg, w, h, "translation")
    for rec in (prev, cur):
        assert set(np.unique(rec["object"]).tolist()) == {-1, 0, 1, 2}
        assert ((rec["hit"] & 3) == 2).any() and np.isnan(rec["pos"]).any()
    assert np.isnan(rgba).any() and np.isinf(rgba).any() and (rgba[..., 3] == 0).any() and (rgba[..., 3] < 0).any()
    # off-screen points and points that stay: the translated view loses some pixels and keeps most
    out = ref.reproject(orc, rgba, prev, cur, ref.VIEW_PARAMS, cam, 0.1, 0.9, 16.0)
    hit = (cur["object"] >= 0) & ((cur["hit"] & 3) != 2)
    carried = out[..., 3] > 0
    assert 0.3 < carried[hit].mean() < 0.98, carried[hit].mean()
    assert (out[..., 3][carried] <= 16.0).all() and (out[..., 3][carried] == 16.0).any() and (out[..., 3][carried] < 16.0).any()  # the clamp, both sides
    assert not carried[~hit].any()
    # behind the previous camera: nothing
    rgba, prev, cur, cam = ref.synthetic(pkg, w, h, "behind")
    assert not ref.reproject(orc, rgba, prev, cur, ref.VIEW_PARAMS, cam, 0.1, 0.9, 16.0).any()


@pytest.mark.parametrize("case", sorted(ref.CAMERAS))
@pytest.mark.parametrize("w,h", [(61, 35), (2, 2), (1, 9), (9, 1), (1, 1)])
def test_math_header_equals_the_numpy_restatement(pkg, orc, driver, case, w, h, tmp_path):
    rgba, prev, cur, cam = ref.synthetic(pkg, w, h, case, seed=w + h)
    for flags, max_history, max_plane, min_dot in ((0, 16.0, 0.1, 0.9), (1, 1000.0, 0.02, 0.99), (0, 2.5, 10.0, -1.0)):
        args = (ref.VIEW_PARAMS, cam, max_plane, min_dot, max_history, flags)
        got = driver(rgba, prev, cur, *args, via_file=(tmp_path / "in.bin") if flags else None)
        want = ref.reproject(orc, rgba, prev, cur, *args)
        assert_same_bits(got, want, f"{case} {w} x {h} flags {flags}")
        if w == 1 or h == 1 or case == "behind":
            assert not got.view(np.uint32).any(), "a one-pixel-wide or -high image and a camera behind the scene carry nothing"
        elif case == "identity" and w > 2 and h > 2:
            assert (got[..., 3] > 0).any()
        glass = (cur["hit"] & 3) == 2
        if not flags:
            assert not got[glass].view(np.uint32).any()
        elif w > 2 and h > 2 and case != "behind":
            assert (got[..., 3][glass] > 0).any()
        assert not got[cur["object"] < 0].view(np.uint32).any() and not got[~np.isfinite(cur["pos"]).all(axis=-1)].view(np.uint32).any()


def test_the_edges_of_the_previous_image(pkg, orc, driver):
    """fx exactly on -1, 0, W - 1 and W (tests/reproject_reference.py, edge_case): history exactly for -1 < fx < W; at fx = -0.5 the one
    tap inside carries all of it; at integer fx the tap with weight 0 changes nothing."""
    rgba, prev, cur, cam, vp, fx = ref.edge_case(pkg)
    got = driver(rgba, prev, cur, vp, cam, 0.01, 0.9, 100.0)
    assert_same_bits(got, ref.reproject(orc, rgba, prev, cur, vp, cam, 0.01, 0.9, 100.0), "edge case")
    has = [bool(got[0, x, 3] > 0) for x in range(len(fx))]
    assert has == [-1 < float(F(f)) < 17 for f in fx] == [False, True, True, True, True, True, True, False, False, True]
    assert_same_bits(got[0, 1:2], rgba[2, 0:1], "fx = -0.5: the tap at column 0")       # w = 0.5 cancels: mean and count of that tap
    assert_same_bits(got[0, 2:3], rgba[2, 0:1], "fx = 0")
    assert_same_bits(got[0, 5:6], rgba[2, 16:17], "fx = W - 1")
    assert_same_bits(got[0, 6:7], rgba[2, 16:17], "fx = W - 0.5")
    assert_same_bits(got[0, 9:10], rgba[2, 8:9], "fx = 8")
    # every other pixel of this identity view sits exactly on its own previous pixel
    assert_same_bits(got[1:], rgba[1:], "identity")


def test_resolve_equals_the_numpy_restatement(pkg, orc, driver):
    rgba = ref.sums(37, 21, 3)
    got = driver.resolve(rgba)
    assert_same_bits(got, ref.resolve(orc, rgba), "resolve")
    assert np.array_equal(got[..., 3].view(np.uint32), rgba[..., 3].view(np.uint32))
    assert not got[..., :3][~(rgba[..., 3] > 0)].view(np.uint32).any()
    ok = (rgba[..., 3] > 0) & np.isfinite(rgba).all(axis=-1)
    assert np.allclose(got[..., :3][ok] * rgba[..., 3:4][ok], rgba[..., :3][ok], rtol=1e-6)
