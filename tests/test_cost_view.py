"""The per-pixel traversal-cost view without a GPU: include/rt_cost.h is plain C, exported by the library and mirrored by
hip.COST_SYMBOLS; rt_render_cost refuses a null context; the heatmap of display.cost_heatmap_srgb8 is exactly its
definition (t = value / scale in fp32, red above 1, grey uint8(t * 255 + 0.5) otherwise)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cost_header_functions():
    text = open(os.path.join(ROOT, "include", "rt_cost.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rt_[a-z_0-9]+)\s*\(", text)))


def test_cost_header_symbols_are_exported_and_listed(pkg, api):
    names = cost_header_functions()
    assert names == ["rt_render_cost"]
    assert sorted(pkg.hip.COST_SYMBOLS) == names, "hip.COST_SYMBOLS is out of sync with include/rt_cost.h"
    assert not set(names) & set(pkg.hip.ABI_SYMBOLS), "rt_cost.h's calls are not rt_abi.h's"
    for n in names:
        assert hasattr(api.lib, n), f"libraytrace_hip.so does not export {n}"


def test_pixel_cost_layout(pkg):
    assert len(pkg.hip.COST_FIELDS) == 8
    header = open(os.path.join(ROOT, "include", "rt_cost.h")).read()
    body = re.search(r"typedef struct RtPixelCost \{(.*?)\} RtPixelCost;", header, flags=re.S).group(1)
    fields = re.findall(r"uint32_t\s+(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert tuple(fields) == pkg.hip.COST_FIELDS  # render_cost's columns are the struct's fields, in order
    assert 'sizeof(RtPixelCost) == 32' in header


def test_cost_header_is_plain_c_and_links_from_a_c_program(pkg, api, tmp_path):
    """rt_cost.h compiles as C99 (pedantic), RtPixelCost is 32 bytes with the fields where the header says, and a C program links
    against libraytrace_hip.so and gets RT_ERR_INVALID_ARG from rt_render_cost(NULL, ...) without a GPU."""
    src = tmp_path / "cost.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "rt_cost.h"
typedef char size_is_32[sizeof(RtPixelCost) == 32 ? 1 : -1];
typedef char first_hit_last[offsetof(RtPixelCost, firstHit) == 28 ? 1 : -1];
typedef char tri_tests_fourth[offsetof(RtPixelCost, triTests) == 12 ? 1 : -1];
int main(void)
{
    RtPixelCost px[1];
    size_is_32 a;
    first_hit_last b;
    tri_tests_fourth c;
    (void)a; (void)b; (void)c;
    if (rt_render_cost(NULL, 1, px, sizeof px) != RT_ERR_INVALID_ARG) return 2;
    if (rt_render_cost(NULL, 0, NULL, 0) != RT_ERR_INVALID_ARG) return 3;
    printf("%s | %s\n", rt_version(), rt_last_error(NULL));
    return 0;
}
''')
    exe = tmp_path / "cost"
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lraytrace_hip", "-Wl,-rpath," + libdir])
    out = subprocess.check_output([str(exe)], text=True)
    assert "raytrace_hip gfx950" in out and "null context" in out


def test_render_cost_refuses_a_null_context(pkg, api):
    buf = np.zeros(8, dtype=np.uint32)
    assert api.render_cost(None, 1, buf.ctypes.data, buf.nbytes) == pkg.abi.RT_ERR_INVALID_ARG
    assert b"null context" in api.last_error(None)


def heatmap_restated(cost, column, scale, flip_y=True):
    """The definition, one pixel at a time."""
    rows, w = cost.shape[:2]
    out = np.zeros((rows, w, 4), dtype=np.uint8)
    for y in range(rows):
        for x in range(w):
            v = np.float32(2 * int(cost[y, x, 1])) if column == "boxTests" else np.float32(cost[y, x, column])
            t = np.float32(v / np.float32(scale))
            if t > np.float32(1):
                out[y, x] = (255, 0, 0, 255)
            else:
                g = np.uint8(np.float32(t * np.float32(255) + np.float32(0.5)))
                out[y, x] = (g, g, g, 255)
    return out[::-1] if flip_y else out


def test_cost_heatmap_matches_its_definition(pkg):
    rng = np.random.default_rng(3)
    cost = rng.integers(0, 400, size=(5, 7, 8), dtype=np.uint64).astype(np.uint32)
    cost[0, 0, 3] = 300          # t == 1 exactly at scale 300: grey 255, not red
    cost[0, 1, 3] = 301          # t > 1: red
    cost[1, 0, 3] = 0
    cost[1, 1, 1] = 150          # boxTests = 300: t == 1 at scale 300
    cost[1, 2, 1] = 151          # boxTests = 302 > 300
    cost[2, 0, 3] = 0xFFFFFFFF   # large values convert to fp32 first
    fields = pkg.hip.COST_FIELDS
    for field in list(fields) + ["boxTests"]:
        column = "boxTests" if field == "boxTests" else fields.index(field)
        for scale in (300, 7.3, 1.0, 1e-3, 1e9):
            for flip in (True, False):
                got = pkg.display.cost_heatmap_srgb8(cost, field, scale, flip_y=flip)
                want = heatmap_restated(cost, column, scale, flip)
                assert got.dtype == np.uint8 and got.shape == (5, 7, 4)
                assert np.array_equal(got, want), (field, scale, flip)
    tri = pkg.display.cost_heatmap_srgb8(cost, "triTests", 300, flip_y=False)
    assert tuple(tri[0, 0]) == (255, 255, 255, 255) and tuple(tri[0, 1]) == (255, 0, 0, 255) and tuple(tri[1, 0]) == (0, 0, 0, 255)
    box = pkg.display.cost_heatmap_srgb8(cost, "boxTests", 300, flip_y=False)
    assert tuple(box[1, 1]) == (255, 255, 255, 255) and tuple(box[1, 2]) == (255, 0, 0, 255)
    # flip_y: top row first, like rt_display_srgb8
    assert np.array_equal(pkg.display.cost_heatmap_srgb8(cost, "segments", 50), pkg.display.cost_heatmap_srgb8(cost, "segments", 50, flip_y=False)[::-1])


def test_cost_heatmap_refuses_bad_input(pkg):
    cost = np.zeros((2, 3, 8), dtype=np.uint32)
    for field, scale in (("nope", 1.0), ("segments", 0.0), ("segments", -1.0), ("segments", float("nan")), ("segments", float("inf"))):
        with pytest.raises(ValueError):
            pkg.display.cost_heatmap_srgb8(cost, field, scale)
    with pytest.raises(ValueError):
        pkg.display.cost_heatmap_srgb8(np.zeros((2, 3, 4), dtype=np.uint32), "segments", 1.0)


def test_rt_render_cost_png_needs_a_scale():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rt_render.py"), "3", "--cost-png", "x.png"], capture_output=True, text=True)
    assert r.returncode == 2 and "--cost-png needs --cost-scale" in r.stderr
