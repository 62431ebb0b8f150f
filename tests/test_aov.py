"""The first-hit feature buffers (include/rt_aov.h) without a GPU: the header is plain C (C99 and C++17), RtPixelAov is 64 bytes
with the same field offsets in C, in the ctypes struct and in the numpy dtype; the library exports both calls and refuses a null
context; display.aov_srgb8 draws exactly its documented formulas."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
FIELDS = ("dst", "normal", "pos", "hit", "albedo", "object", "emission", "triangle")
OFFSETS = {"dst": 0, "normal": 4, "pos": 16, "hit": 28, "albedo": 32, "object": 44, "emission": 48, "triangle": 60}


def aov_header_functions():
    text = open(os.path.join(INCLUDE, "rt_aov.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rt_[a-z_0-9]+)\s*\(", text)))


# ---------------------------------------------------------------- 1. the header and the three layouts
@pytest.mark.parametrize("lang", ["c99", "c++17"])
def test_header_compiles_and_has_the_documented_layout(lang, tmp_path):
    cxx = lang.startswith("c++")
    src = tmp_path / ("aov.cpp" if cxx else "aov.c")
    checks = "\n".join(f"typedef char at_{f}[offsetof(RtPixelAov, {f}) == {o} ? 1 : -1];" for f, o in OFFSETS.items())
    src.write_text('#include <stddef.h>\n#include "rt_aov.h"\ntypedef char size_is_64[sizeof(RtPixelAov) == 64 ? 1 : -1];\n' + checks +
                   "\nint use(RtContext* c, RtPixelAov* p) { return rt_render_aov(c, 1, p, sizeof *p) + rt_render_aov_to_device(c, 1, p, sizeof *p); }\n")
    cmd = ["g++", "-x", "c++"] if cxx else ["gcc", "-x", "c"]
    subprocess.check_call(cmd + [f"-std={lang}", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(src)])


def test_ctypes_struct_and_numpy_dtype_are_the_same_64_bytes(pkg):
    abi = pkg.abi
    assert C.sizeof(abi.RtPixelAov) == 64 and abi.AOV_DTYPE.itemsize == 64
    assert tuple(n for n, _ in abi.RtPixelAov._fields_) == FIELDS == abi.AOV_DTYPE.names
    for f, off in OFFSETS.items():
        assert getattr(abi.RtPixelAov, f).offset == off, f
        assert abi.AOV_DTYPE.fields[f][1] == off, f
        assert getattr(abi.RtPixelAov, f).size == abi.AOV_DTYPE.fields[f][0].itemsize, f
    # one record written through ctypes reads back through the dtype
    rec = abi.RtPixelAov(dst=2.5, normal=(0.0, 1.0, 0.0), pos=(1.0, 2.0, 3.0), hit=0x102, albedo=(0.25, 0.5, 0.75), object=7,
                         emission=(4.0, 0.0, 0.5), triangle=-1)
    a = np.frombuffer(bytes(rec), dtype=abi.AOV_DTYPE)[0]
    assert a["dst"] == 2.5 and a["normal"].tolist() == [0, 1, 0] and a["pos"].tolist() == [1, 2, 3] and a["hit"] == 0x102
    assert a["albedo"].tolist() == [0.25, 0.5, 0.75] and a["object"] == 7 and a["emission"].tolist() == [4, 0, 0.5] and a["triangle"] == -1
    assert a["hit"] & abi.AOV_HIT_CLASS_MASK == 2 and a["hit"] & abi.AOV_HIT_BACKFACE


# ---------------------------------------------------------------- 2. exports, null context
def test_aov_header_symbols_are_exported_and_listed(pkg, api):
    names = aov_header_functions()
    assert names == ["rt_render_aov", "rt_render_aov_to_device"]
    assert sorted(pkg.hip.AOV_SYMBOLS) == names, "hip.AOV_SYMBOLS is out of sync with include/rt_aov.h"
    assert not set(names) & set(pkg.hip.ABI_SYMBOLS), "rt_aov.h's calls are not rt_abi.h's"
    for n in names:
        assert hasattr(api.lib, n), f"libraytrace_hip.so does not export {n}"


def test_both_calls_refuse_a_null_context(pkg, api):
    buf = np.zeros(1, dtype=pkg.abi.AOV_DTYPE)
    for call in (api.render_aov, api.render_aov_to_device):
        assert call(None, 1, buf.ctypes.data, buf.nbytes) == pkg.abi.RT_ERR_INVALID_ARG
        assert b"null context" in api.last_error(None)
        assert call(None, 0, None, 0) == pkg.abi.RT_ERR_INVALID_ARG


# ---------------------------------------------------------------- 3. display.aov_srgb8
def records(pkg):
    """2 rows x 3 columns, rows bottom-up.  Row 0: a miss with a sky colour, sphere 0 at depth 2, model 5 at depth 4 (back face).
    Row 1: a miss without sky, glass sphere 1 at depth 3, model 5 at depth 6."""
    a = np.zeros((2, 3), dtype=pkg.abi.AOV_DTYPE)
    a["object"] = -1
    a["triangle"] = -1
    a["dst"] = np.inf
    a["albedo"][0, 0] = (0.5, 0.25, 1.0)

    def hit(y, x, dst, n, alb, em, cls, obj, tri):
        a[y, x] = (dst, n, (0, 0, dst), cls, alb, obj, em, tri)
    hit(0, 1, 2.0, (0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1, 0, -1)
    hit(0, 2, 4.0, (-1.0, 0.0, 0.0), (0.0, 0.5, 2.0), (0.25, 0.0, 0.0), 1 | 0x100, 5, 17)
    hit(1, 1, 3.0, (0.0, 0.0, 1.0), (0.2, 0.2, 0.2), (0.0, 1.0, 0.0), 2, 1, -1)
    hit(1, 2, 6.0, (0.6, 0.0, -0.8), (1.0, 1.0, 1.0), (0.0, 0.0, 8.0), 1, 5, 18)
    return a


def q(t):
    return int(np.uint8(np.clip(np.float32(t), 0, 1) * np.float32(255) + np.float32(0.5)))


def test_aov_srgb8_every_channel(pkg):
    d = pkg.display
    a = records(pkg)
    assert d.AOV_CHANNELS == ("normal", "albedo", "emission", "depth", "object")
    for ch in d.AOV_CHANNELS:
        img = d.aov_srgb8(a, ch, flip_y=False)
        assert img.shape == (2, 3, 4) and img.dtype == np.uint8 and (img[..., 3] == 255).all(), ch
        assert np.array_equal(d.aov_srgb8(a, ch), img[::-1]), ch  # flip_y (the default): top row first
    n = d.aov_srgb8(a, "normal", flip_y=False)
    assert n[0, 0, :3].tolist() == [q(0.5)] * 3 == [128] * 3  # a miss: n = 0
    assert n[0, 1, :3].tolist() == [128, 255, 128] and n[0, 2, :3].tolist() == [0, 128, 128]
    assert n[1, 2, :3].tolist() == [q(np.float32(0.6) * np.float32(0.5) + np.float32(0.5)), 128, q(np.float32(-0.8) * np.float32(0.5) + np.float32(0.5))]
    alb = d.aov_srgb8(a, "albedo", flip_y=False)
    assert alb[0, 0, :3].tolist() == [128, 64, 255]  # the sky colour of a miss
    assert alb[1, 0, :3].tolist() == [0, 0, 0] and alb[0, 1, :3].tolist() == [255, 0, 0]
    assert alb[0, 2, :3].tolist() == [0, 128, 255]  # clipped at 1
    assert alb[1, 1, :3].tolist() == [q(0.2)] * 3
    em = d.aov_srgb8(a, "emission", flip_y=False)
    assert em[0, 2, :3].tolist() == [64, 0, 0] and em[1, 1, :3].tolist() == [0, 255, 0] and em[1, 2, :3].tolist() == [0, 0, 255]
    assert not em[:, 0, :3].any()
    dep = d.aov_srgb8(a, "depth", flip_y=False)  # finite hits: 2 .. 6
    assert not dep[:, 0, :3].any()  # misses are black
    assert [dep[0, 1, 0], dep[1, 1, 0], dep[0, 2, 0], dep[1, 2, 0]] == [0, q(0.25), q(0.5), 255]
    assert (dep[..., 0] == dep[..., 1]).all() and (dep[..., 0] == dep[..., 2]).all()
    dep = d.aov_srgb8(a, "depth", flip_y=False, depth_range=(0.0, 4.0))
    assert [dep[0, 1, 0], dep[1, 1, 0], dep[0, 2, 0], dep[1, 2, 0]] == [q(0.5), q(0.75), 255, 255]
    obj = d.aov_srgb8(a, "object", flip_y=False)
    assert not obj[:, 0, :3].any()
    assert (obj[0, 2] == obj[1, 2]).all()  # the same object, the same colour
    seen = {tuple(obj[0, 1, :3]), tuple(obj[1, 1, :3]), tuple(obj[0, 2, :3])}
    assert len(seen) == 3 and all(min(c) >= 64 for c in seen)
    for o, px in ((0, obj[0, 1]), (1, obj[1, 1]), (5, obj[0, 2])):  # the documented hash
        h = ((o + 1) * 2654435761) & 0xffffffff
        assert px[:3].tolist() == [64 + ((h >> s) & 0xff) * 3 // 4 for s in (0, 8, 16)]


def test_aov_srgb8_constant_depth_no_hits_and_bad_input(pkg):
    d = pkg.display
    a = records(pkg)
    hit = (a["hit"] & 3) != 0
    a["dst"][hit] = 3.0
    with np.errstate(all="raise"):  # no division by zero
        dep = d.aov_srgb8(a, "depth", flip_y=False)
        assert not dep[..., :3].any() and (dep[..., 3] == 255).all()
        dep = d.aov_srgb8(a, "depth", flip_y=False, depth_range=(3.0, 3.0))
        assert not dep[..., :3].any()
        none = np.zeros((2, 2), dtype=pkg.abi.AOV_DTYPE)
        none["dst"] = np.inf
        none["object"] = -1
        for ch in d.AOV_CHANNELS:
            img = d.aov_srgb8(none, ch)
            assert img.shape == (2, 2, 4) and (img[..., 3] == 255).all()
            assert (img[..., :3] == (128 if ch == "normal" else 0)).all(), ch
        nan = records(pkg)
        nan["normal"][0, 1] = np.nan  # the NaN ray of a one-pixel-wide image
        nan["dst"][0, 1] = np.nan
        assert d.aov_srgb8(nan, "normal", flip_y=False)[0, 1, :3].tolist() == [0, 0, 0]
        assert d.aov_srgb8(nan, "depth", flip_y=False)[0, 1, :3].tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        d.aov_srgb8(a, "cost")
    with pytest.raises(ValueError):
        d.aov_srgb8(np.zeros((2, 3, 8), dtype=np.uint32), "normal")
